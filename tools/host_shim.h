// What the tools/*_host_check.cpp programs share: enough of HIP to run a kernel header of csrc/ block by block on host
// threads under the address and undefined-behaviour sanitisers.  __global__, __device__, __forceinline__ and
// __launch_bounds__ expand to plain C++, __shared__ to a static array (so one block runs at a time), threadIdx / blockIdx
// are thread-local, __syncthreads is a pthread barrier.  A program includes this header, adds what its kernels need
// beyond it (atomic-add macros, float2 / float4, min / max), then includes the kernel header.
#pragma once

#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <limits>
#include <vector>

#include "../include/windsr_hip.h"

struct Dim3 {
  unsigned x = 1, y = 1, z = 1;
};
static thread_local Dim3 threadIdx, blockIdx;
static Dim3 gridDim;
static pthread_barrier_t g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&g_barrier); }
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __shared__ static
// the integer add behind a kernel header's *_LDS_ADD / *_GLOBAL_ADD macros, for 32-bit counters and 64-bit tables alike
#define HOST_SHIM_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)

namespace {

std::function<void()> g_body;

void* worker(void* arg) {
  threadIdx.x = (unsigned)(intptr_t)arg;
  for (unsigned bz = 0; bz < gridDim.z; ++bz)
    for (unsigned by = 0; by < gridDim.y; ++by)
      for (unsigned bx = 0; bx < gridDim.x; ++bx) {
        blockIdx.x = bx, blockIdx.y = by, blockIdx.z = bz;
        g_body();
        pthread_barrier_wait(&g_barrier);  // (LDS is one static array: a block at a time)
      }
  return nullptr;
}

// a grid of gx x gy x gz blocks of nt threads
void launch(int nt, unsigned gx, unsigned gy, unsigned gz, std::function<void()> body) {
  gridDim.x = gx, gridDim.y = gy, gridDim.z = gz;
  g_body = std::move(body);
  pthread_barrier_init(&g_barrier, nullptr, (unsigned)nt);
  std::vector<pthread_t> th((size_t)nt);
  for (int t = 0; t < nt; ++t) pthread_create(&th[t], nullptr, worker, (void*)(intptr_t)t);
  for (int t = 0; t < nt; ++t) pthread_join(th[t], nullptr);
  pthread_barrier_destroy(&g_barrier);
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
double uniform() {  // (-1, 1)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_rng >> 11) / 9007199254740992.0) * 2.0 - 1.0;
}

template <class T> void dump(FILE* f, const T* p, size_t n) {
  if (f && fwrite(p, sizeof(T), n, f) != n) abort();
}

}  // namespace
