# The block-sparse Schur complement tests' own program (tests/test_schur_sparse.py):
#   make -f schur_sparse.mk driver   the structure driver under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
CSE_H := $(REPO)/include/cse.h
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/schur_sparse_driver

build/schur_sparse_driver: schur_sparse_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp $(CSRC)/plan.hpp \
    $(CSRC)/host_shared.hpp $(CSE_H)
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ schur_sparse_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp

.PHONY: driver
