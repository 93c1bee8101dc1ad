// hip/hip_runtime.h stand-in for tests/test_select_kernel_on_host.py: runs the SOURCE TEXT of a small HIP kernel on the CPU, one std::thread
// per lane -- __syncthreads is a barrier over the workgroup, __shfl_xor an exchange through memory between two barriers over the wave's 64
// lanes, __shared__ a static.  Enough for csrc/hmpc_select.hip (no LDS atomics, no early return of part of a workgroup); not a HIP runtime.
#pragma once
#include <barrier>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
inline thread_local dim3 threadIdx, blockIdx, blockDim;
inline std::barrier<> *g_block_barrier;
inline std::vector<std::unique_ptr<std::barrier<>>> g_wave_barrier;
inline unsigned long long g_xchg[1024];
inline void __syncthreads() { g_block_barrier->arrive_and_wait(); }
template <class T> inline T __shfl_xor(T v, int mask, int width) {
  static_assert(sizeof(T) <= 8, "");
  const int tid = threadIdx.x, wave = tid / 64;
  unsigned long long bits = 0; memcpy(&bits, &v, sizeof(T));
  g_xchg[tid] = bits;
  g_wave_barrier[wave]->arrive_and_wait();
  unsigned long long got = g_xchg[(tid & ~63) | ((tid & 63) ^ mask)];
  g_wave_barrier[wave]->arrive_and_wait();
  T out; memcpy(&out, &got, sizeof(T)); return out;
}
inline long long __double_as_longlong(double v) { long long b; memcpy(&b, &v, 8); return b; }
inline double __longlong_as_double(long long b) { double v; memcpy(&v, &b, 8); return v; }
inline hipError_t hipGetLastError() { return hipSuccess; }
template <class F, class... A> void emu_launch(F kernel, dim3 grid, dim3 block, A... args) {
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bb(block.x); g_block_barrier = &bb;
    g_wave_barrier.clear();
    for (unsigned w = 0; w < (block.x + 63) / 64; ++w) g_wave_barrier.emplace_back(new std::barrier<>(64));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t) th.emplace_back([=]() {
      threadIdx = dim3(t), blockIdx = dim3(b), blockDim = block;
      kernel(args...);  // (a kernel may return early only with its whole workgroup, before any barrier)
    });
    for (auto &x : th) x.join();
  }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
