// Host stand-in for <hip/hip_runtime.h>, for tests/test_shelter_emulation.py only: just enough to compile
// ssrs_amd/csrc/shelter.hip with g++ and run its kernel on the CPU -- one block at a time, one OS thread per GPU
// thread, __syncthreads() a pthread barrier, __shared__ a function-local static.  It checks the kernel's logic
// (tiling, halo staging, sample tables, batching) where no GPU is present; it says nothing about the device's
// arithmetic or speed, which the gpu-marked tests cover.
#pragma once
#include <pthread.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static

typedef void *hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
inline const char *hipGetErrorString(hipError_t) { return "host emulation"; }
inline hipError_t hipGetLastError() { return hipSuccess; }

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct EmuIndex {
    unsigned x = 0, y = 0, z = 0;
};
inline thread_local EmuIndex threadIdx;
inline EmuIndex blockIdx, gridDim, blockDim;
inline pthread_barrier_t emu_barrier;
inline void __syncthreads() { pthread_barrier_wait(&emu_barrier); }
inline double __builtin_amdgcn_rsq(double s) { return 1.0 / std::sqrt(s); }

inline void emu_launch(dim3 grid, dim3 block, const std::function<void()> &kernel)
{
    gridDim.x = grid.x;
    blockDim.x = block.x;
    for (unsigned b = 0; b < grid.x; ++b) {
        blockIdx.x = b;
        pthread_barrier_init(&emu_barrier, nullptr, block.x);
        std::vector<std::thread> threads;
        for (unsigned t = 0; t < block.x; ++t)
            threads.emplace_back([&kernel, t] {
                threadIdx.x = t;
                kernel();
            });
        for (auto &t : threads) t.join();
        pthread_barrier_destroy(&emu_barrier);
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })
