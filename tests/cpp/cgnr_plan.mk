# The CGNR block-table test's own program (tests/test_cgnr_solve.py):
#   make -f cgnr_plan.mk driver   the plan driver under ASan + UBSan (g++, no HIP)
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
CSE_H := $(REPO)/include/cse.h
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread

driver: build/cgnr_plan_driver

build/cgnr_plan_driver: cgnr_plan_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp $(CSRC)/plan.hpp \
    $(CSRC)/host_shared.hpp $(CSE_H)
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ cgnr_plan_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp

.PHONY: driver
