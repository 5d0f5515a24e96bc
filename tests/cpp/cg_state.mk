# The device PCG tests' own program (tests/test_schur_solve.py):
#   make -f cg_state.mk driver   csrc/cg_state.hpp's transitions under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/cg_state_driver

build/cg_state_driver: cg_state_driver.cpp $(CSRC)/cg_state.hpp
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ cg_state_driver.cpp

.PHONY: driver
