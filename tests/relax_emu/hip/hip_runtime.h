// Host stand-in for <hip/hip_runtime.h>, just large enough to compile abx_amd/csrc/relax.hip with g++ and run relax_kernel on CPU threads
// (tests/test_relax_host.py): one std::thread per GPU thread of a workgroup, __syncthreads = a barrier of the 1024 threads, a wave
// shuffle = an exchange through memory between the 64 threads of a wave.  Test infrastructure only.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3 { int x, y, z; dim3(int a = 1, int b = 1, int c = 1) : x(a), y(b), z(c) {} };
struct EmuIdx { int x, y, z; };
extern thread_local EmuIdx threadIdx, blockIdx;
extern std::barrier<>* emu_block_barrier;
extern std::barrier<>* emu_wave_barrier[16];
extern double emu_shuffle[1024];
extern unsigned char* emu_lds;
inline void __syncthreads() { emu_block_barrier->arrive_and_wait(); }
template <class T> inline T __shfl_xor(T v, int o, int) {
    memcpy(&emu_shuffle[threadIdx.x], &v, sizeof(T));
    emu_wave_barrier[threadIdx.x >> 6]->arrive_and_wait();
    T r;
    memcpy(&r, &emu_shuffle[threadIdx.x ^ o], sizeof(T));
    emu_wave_barrier[threadIdx.x >> 6]->arrive_and_wait();
    return r;
}
inline float __cosf(float x) { return cosf(x); }
inline float __sinf(float x) { return sinf(x); }
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
#define hipLaunchKernelGGL(...) do {} while (0)
