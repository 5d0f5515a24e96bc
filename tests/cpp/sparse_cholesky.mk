# The block-sparse Cholesky tests' own program (tests/test_sparse_cholesky.py):
#   make -f sparse_cholesky.mk driver   the plan and its host replay under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
CSE_H := $(REPO)/include/cse.h
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/sparse_cholesky_driver

build/sparse_cholesky_driver: sparse_cholesky_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp $(CSRC)/plan.hpp \
    $(CSRC)/host_shared.hpp $(CSE_H)
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ sparse_cholesky_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp

.PHONY: driver
