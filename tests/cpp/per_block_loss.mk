# The per-block loss tests' own programs (tests/test_per_block_loss.py,
# tests/test_per_block_loss_facade_gpu.py):
#   make -f per_block_loss.mk driver   the planner driver under ASan + UBSan (g++, no HIP)
#   make -f per_block_loss.mk facade   the C++ facade test against libcse.so and the oracle
REPO := $(abspath ../..)
CXX ?= g++
CSRC := $(REPO)/ceres-solver-cuda_amd/csrc
CSE_H := $(REPO)/include/cse.h
ASAN_GXX := -O1 -g -std=c++17 -Wall -Wextra -fno-omit-frame-pointer -fsanitize=address,undefined \
            -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread
INC := -I$(REPO)/ceres-solver-cuda_amd/include -I$(REPO)/oracle
LIBS := -L$(REPO)/ceres-solver-cuda_amd/lib -lcse -L$(REPO)/oracle/build -loracle \
        -Wl,-rpath,$(REPO)/ceres-solver-cuda_amd/lib -Wl,-rpath,$(REPO)/oracle/build \
        -Wl,-rpath,/opt/rocm/lib

driver: build/per_block_loss_driver
facade: build/test_per_block_loss

build/per_block_loss_driver: per_block_loss_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp $(CSRC)/plan.hpp \
    $(CSRC)/host_shared.hpp $(CSE_H)
	@mkdir -p build
	$(CXX) $(ASAN_GXX) -o $@ per_block_loss_driver.cpp $(CSRC)/layout.cpp $(CSRC)/plan.cpp

build/test_per_block_loss: test_per_block_loss.cpp \
    $(REPO)/ceres-solver-cuda_amd/include/ceres_amd/problem_cuda.h $(CSE_H)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -Wall -Wextra $(INC) -o $@ $< $(LIBS)

.PHONY: driver facade
