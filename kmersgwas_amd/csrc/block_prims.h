// block_prims.h — what a 256-thread block (four waves) adds up together, once: the block sum, the exclusive scan with a running
// carry, and the filters' tested-row count. Everything is __forceinline__ and works on the caller's registers and on LDS words
// the caller names; each primitive has ONE barrier, behind its LDS writes. A caller that uses the same LDS words again - in a
// loop, or for a second primitive - puts its own barrier between the reads of one use and the writes of the next.
#pragma once
#include "kernels.h"

namespace kgwas {

template <class T>
__device__ __forceinline__ T wave_sum(T v) {  // every lane gets the sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// v[i] = the sum of v[i] over the block's 256 threads, for every thread. red: 4 * N words of LDS.
template <class T, int N>
__device__ __forceinline__ void block_sum(T (&v)[N], T* red) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; i++) {
        v[i] = wave_sum(v[i]);
        if (lane == 0u) red[wave * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = red[i] + red[N + i] + red[2 * N + i] + red[3 * N + i];
}
template <class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    T a[1] = {v};
    block_sum(a, red);
    return a[0];
}

// carry + the sum of v over the threads below this one; carry (the same register value in every thread) moves on by the
// block's total. part: 4 words of LDS.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t& carry, uint32_t* part) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if ((int)lane >= d) incl += t;
    }
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint32_t o = carry + incl - v;
    for (uint32_t k = 0; k < wave; k++) o += part[k];
    carry += part[0] + part[1] + part[2] + part[3];
    return o;
}

// the MAC-passing rows a wave's lanes counted, into the launch's sharded counter (one atomic per wave)
__device__ __forceinline__ void filter_add_tested(unsigned long long* tested, uint32_t v, uint32_t lane) {
    if (!tested) return;
    v = wave_sum(v);
    if (lane == 0u && v) atomicAdd(&tested[blockIdx.x % TESTED_SHARDS], (unsigned long long)v);
}

}  // namespace kgwas
