// kmer_windows.h — the k-base windows of a resident base stream, shared by count_kernels.hip (count_kmers_with_strand),
// locate_kernels.hip (locate_kmers) and fetch_kernels.hip (fetch_reads): the tile they walk, a base's 2-bit code, sixteen positions packed from one 16-byte load, and
// the reverse complement of a code. The base stream is bytes; A C G T (either case) are bases, every other byte separates.
//
// The tile: a workgroup of 256 lanes takes 4096 positions, 16 per lane. Each lane packs its 16 bases into 32 bits of 2-bit codes
// (first base in the top bits) and 16 validity bits; the packed tile and a halo of 32 positions go to LDS, from where a lane takes
// the two entries behind its own: 48 positions in registers cover its 16 windows of up to 31 bases.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kgwas {

constexpr uint32_t CK_BLOCK = 256;
constexpr uint32_t CK_RUN = 16;                    // positions per lane
constexpr uint32_t CK_TILE = CK_BLOCK * CK_RUN;    // positions per workgroup and step
constexpr uint32_t CK_PACKS = CK_BLOCK + 2;        // packed entries per tile: its own and a halo of 32 positions >= k - 1

// 2-bit code of a base, 4 for a separator
__device__ __forceinline__ uint32_t ck_code(uint32_t c) {
    c &= 0xDFu;  // (lower case)
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// 16 positions from p on: codes (position i in bits 31-2i, 30-2i) and validity (bit i); positions at or behind n are separators
__device__ __forceinline__ void ck_pack(const uint8_t* bases, uint64_t n, uint64_t p, bool aligned, uint32_t& codes, uint32_t& valid) {
    uint32_t w[4] = {0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au};
    if (p + 16 <= n && aligned) {
        const uint4 v = *reinterpret_cast<const uint4*>(bases + p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if (p < n) {
        const uint32_t m = (uint32_t)min((uint64_t)16, n - p);
        for (uint32_t i = 0; i < m; i++) w[i >> 2] = (w[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | ((uint32_t)bases[p + i] << (8 * (i & 3)));
    }
    codes = 0, valid = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t c = ck_code((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
        codes |= (c & 3u) << (30 - 2 * i);
        valid |= (uint32_t)(c < 4u) << i;
    }
}

// the reverse complement of a k-base code (kmer_reverse_complement, src/kmer_general.h:102-109)
__device__ __forceinline__ uint64_t ck_revcomp(uint64_t a, uint32_t k) {
    uint64_t x = ((uint64_t)__brev((uint32_t)a) << 32) | __brev((uint32_t)(a >> 32));  // all 64 bits reversed
    x = ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);       // and each pair set right again
    return (~x) >> (64 - 2 * k);
}

// The base that enters a lane's window at its position q (0..47): positions 0-31 lie in X_hi (first base in the top bits), 32-47
// in the top half of X_lo.
__device__ __forceinline__ uint64_t ck_base_at(uint64_t X_hi, uint64_t X_lo, uint32_t q) {
    return q < 32 ? (X_hi >> (62 - 2 * q)) & 3 : (X_lo >> (62 - 2 * (q - 32))) & 3;
}

// A lane's windows of the tile at t0: per_window(j, a) for window j (position t0 + 16 tid + j < n_win, all k bases valid) with
// code a. Returns their number. The tile's packed positions go through s_codes / s_valid; the caller's barrier ends the tile.
template <class F>
__device__ __forceinline__ uint32_t ck_lane_windows(const uint8_t* bases, uint64_t n_buf, uint64_t n_win, uint64_t t0, int aligned, uint32_t k,
                                                    uint32_t* s_codes, uint32_t* s_valid, F&& per_window) {
    const uint32_t tid = threadIdx.x;
    uint32_t c0, v0;
    ck_pack(bases, n_buf, t0 + (uint64_t)tid * CK_RUN, aligned, c0, v0);
    s_codes[tid] = c0, s_valid[tid] = v0;
    if (tid < 2) {
        uint32_t ch, vh;
        ck_pack(bases, n_buf, t0 + CK_TILE + (uint64_t)tid * CK_RUN, aligned, ch, vh);
        s_codes[CK_BLOCK + tid] = ch, s_valid[CK_BLOCK + tid] = vh;
    }
    __syncthreads();
    const uint64_t X_hi = ((uint64_t)c0 << 32) | s_codes[tid + 1], X_lo = (uint64_t)s_codes[tid + 2] << 32;
    const uint64_t V = (uint64_t)v0 | ((uint64_t)s_valid[tid + 1] << 16) | ((uint64_t)s_valid[tid + 2] << 32);
    const uint64_t kmask = (1ull << k) - 1, cmask = (1ull << (2 * k)) - 1;
    const uint64_t p0 = t0 + (uint64_t)tid * CK_RUN;
    uint64_t a = X_hi >> (64 - 2 * k);
    uint32_t n_valid = 0;
#pragma unroll
    for (uint32_t j = 0; j < CK_RUN; j++) {
        if (((V >> j) & kmask) == kmask && p0 + j < n_win) {
            n_valid++;
            per_window(j, a);
        }
        a = ((a << 2) | ck_base_at(X_hi, X_lo, j + k)) & cmask;  // the base at position j + k comes in
    }
    return n_valid;
}

}  // namespace kgwas
