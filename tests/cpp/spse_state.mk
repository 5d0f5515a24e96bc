# The power series expansion tests' own program (tests/test_schur_spse.py):
#   make -f spse_state.mk driver   csrc/spse_state.hpp's transitions under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/spse_state_driver

build/spse_state_driver: spse_state_driver.cpp $(CSRC)/spse_state.hpp $(CSRC)/cg_state.hpp
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ spse_state_driver.cpp

.PHONY: driver
