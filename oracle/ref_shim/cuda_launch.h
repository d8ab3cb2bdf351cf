// oracle/ref_shim/cuda_launch.h — stand-in for what nvcc gives a .cu file without being asked: the launch coordinates of a kernel and
// the two runtime names that the text of main.cu above `int main(` uses (oracle/Makefile, target `ref`; oracle/ref_main_capi.cpp).
// Test infrastructure only; our own text, nothing of CUDA's.
//
// A "launch" on the host is a plain call of the __global__ function with threadIdx / blockIdx / blockDim set by the caller first.
// The driver runs one thread per call: blockDim = (1, 1, 1), threadIdx = (0, 0, 0), blockIdx = (i, j, 0) is pixel (i, j).
#pragma once
#include "cuda_fp16.h"

struct uint3 {
    unsigned int x, y, z;
};
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

static uint3 threadIdx = {0, 0, 0};
static uint3 blockIdx = {0, 0, 0};
static dim3 blockDim(1, 1, 1);

typedef int cudaError_t;
static inline cudaError_t cudaDeviceReset() { return 0; }
