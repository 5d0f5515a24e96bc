# The dense Cholesky tests' own program (tests/test_dense_cholesky.py):
#   make -f dense_cholesky.mk driver   the plan and blocked-order driver under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
CSE_H := $(REPO)/include/cse.h
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/dense_cholesky_driver

build/dense_cholesky_driver: dense_cholesky_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp $(CSRC)/plan.hpp \
    $(CSRC)/host_shared.hpp $(CSE_H)
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ dense_cholesky_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp

.PHONY: driver
