// locate_kernels.hip — device side of locate_kmers (locate.cpp): the windows of a resident base stream that
// spell a query k-mer, or its reverse complement, with at most d <= 1 mismatching bases.
//
// The windows are count_kernels.hip's (kmer_windows.h): a workgroup of 256 lanes takes a tile of 4096 positions, a lane rolls the
// codes of its 16 windows out of 48 packed positions. Only the window's own code is needed: the queries' PATTERNS hold both
// strands, (f_i, +) and, unless r_i == f_i, (r_i, -), as sorted lists that stay on the device (kernels.h, LocateList).
//   d = 0: one list sorted by code. A window looks its code up; an equal entry is a hit.
//   d = 1: H sorted by the pattern's first hh = ceil(k / 2) bases, L by its last lh = floor(k / 2). A window looks its first half up
//          in H: every candidate that differs from it in h <= 1 bases is a hit. Then its last half in L: a candidate is a hit iff
//          h == 1 and the differing base lies in the first half (the others have an equal first half and were met in H). A pair
//          that differs in at most one base has an equal first or an equal last half, so every hit is met, and exactly once.
// A list's splitters sit in LDS (sorted_search.h); the range of equal half keys is walked by the lane that owns the window, however
// long it is. h and the differing base come from the XOR of the two codes folded to one bit per base: a popcount and a count of
// leading zeros.
//
// Records leave the way ld_kernels.hip's proxy records do: count per tile, scan, write - in (pos, kmer, strand) order, the same
// bytes in every run. Within a range the entries are in (kmer, strand) order, so a window's hits are the merge of its two walks.
// The write kernel numbers a tile's records from boff[tile] and stores those of the window [win_lo, win_lo + cap) to
// rec[number - win_lo]: no store is made past rec[cap - 1].
#include "block_prims.h"
#include "kernels.h"
#include "kmer_windows.h"
#include "sorted_search.h"

namespace kgwas {

namespace {

// What a tile's kernels share: the splitters in LDS, the packed tile, and the shape of the search.
struct LkShape {
    uint32_t k, d, hh, lh;
};

// The candidates of one list for one window, in list order: the entries whose half key is the window's. next() moves to the next
// one that is a hit and leaves its id (kmer << 1 | strand), h and offset.
struct LkWalk {
    const LocateList& l;
    uint64_t i, key;
    uint32_t id = 0, h = 0, off = 0;
    __device__ __forceinline__ LkWalk(const LocateList& list, const uint64_t* spl, uint64_t key_) : l(list), key(key_) {
        i = fk_list_bound<false>(spl, list.ns, list.keys, list.n, list.B, key_);
    }
    // second: the walk through L, which takes only what H cannot have met
    __device__ __forceinline__ bool next(uint64_t a, const LkShape& s, bool second) {
        while (i < l.n && l.keys[i] == key) {
            const uint64_t x = a ^ l.codes[i];
            const uint64_t y = (x | (x >> 1)) & 0x5555555555555555ull;  // one bit per differing base
            const uint32_t hm = (uint32_t)__popcll(y);
            id = l.ids[i++];
            // the first differing base, from the window's first base on (0-based): bit 2 j of y is base k - 1 - j
            const uint32_t at = hm ? s.k - 1u - (63u - (uint32_t)__clzll((long long)y)) / 2u : 0u;
            if (second ? (hm == 1u && at < s.hh) : hm <= 1u) {
                h = hm, off = hm ? at + 1u : 0u;
                return true;
            }
        }
        return false;
    }
};

// emit(id, h, offset) for every hit of the window with code a, in id order
template <class F>
__device__ __forceinline__ void lk_window_hits(uint64_t a, const LkShape& s, const LocateList& H, const uint64_t* splH, const LocateList& L,
                                               const uint64_t* splL, F&& emit) {
    LkWalk wh(H, splH, s.d ? a >> (2u * s.lh) : a);
    bool has_h = wh.next(a, s, false);
    if (!s.d) {
        for (; has_h; has_h = wh.next(a, s, false)) emit(wh.id, wh.h, wh.off);
        return;
    }
    LkWalk wl(L, splL, a & ((1ull << (2u * s.lh)) - 1ull));
    bool has_l = wl.next(a, s, true);
    while (has_h || has_l) {
        if (has_h && (!has_l || wh.id < wl.id)) {
            emit(wh.id, wh.h, wh.off);
            has_h = wh.next(a, s, false);
        } else {
            emit(wl.id, wl.h, wl.off);
            has_l = wl.next(a, s, true);
        }
    }
}

__device__ __forceinline__ void lk_load_splitters(const LocateList& H, const LocateList& L, uint64_t* s_splH, uint64_t* s_splL) {
    for (uint32_t i = threadIdx.x; i < H.ns; i += CK_BLOCK) s_splH[i] = H.spl[i];
    for (uint32_t i = threadIdx.x; i < L.ns; i += CK_BLOCK) s_splL[i] = L.spl[i];
    __syncthreads();
}

// bcnt[tile] = the records of the tile; *windows += its windows of k bases
__global__ void __launch_bounds__(CK_BLOCK) lk_count_kernel(const uint8_t* __restrict__ bases, uint64_t n_buf, uint64_t n_win, LkShape s, LocateList H,
                                                            LocateList L, int aligned, uint32_t n_tiles, uint32_t* bcnt,
                                                            unsigned long long* windows) {
    __shared__ uint64_t s_splH[LOCATE_SPLITTERS], s_splL[LOCATE_SPLITTERS];
    __shared__ uint32_t s_codes[CK_PACKS], s_valid[CK_PACKS], red[8];
    lk_load_splitters(H, L, s_splH, s_splL);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t v[2] = {0u, 0u};
        v[1] = ck_lane_windows(bases, n_buf, n_win, (uint64_t)tile * CK_TILE, aligned, s.k, s_codes, s_valid, [&](uint32_t, uint64_t a) {
            lk_window_hits(a, s, H, s_splH, L, s_splL, [&](uint32_t, uint32_t, uint32_t) { v[0]++; });
        });
        block_sum(v, red);
        if (threadIdx.x == 0) {
            bcnt[tile] = v[0];
            if (v[1]) atomicAdd(windows, (unsigned long long)v[1]);
        }
        __syncthreads();  // the tile's LDS words are written again in the next turn
    }
}

// the records numbered [win_lo, win_lo + cap) among those of the tiles [tile0, tile1), to rec[number - win_lo]
__global__ void __launch_bounds__(CK_BLOCK) lk_write_kernel(const uint8_t* __restrict__ bases, uint64_t n_buf, uint64_t n_win, LkShape s, LocateList H,
                                                            LocateList L, int aligned, uint32_t tile0, uint32_t tile1, const uint32_t* boff,
                                                            uint32_t win_lo, uint32_t cap, uint64_t pos0, uint4* rec) {
    __shared__ uint64_t s_splH[LOCATE_SPLITTERS], s_splL[LOCATE_SPLITTERS];
    __shared__ uint32_t s_codes[CK_PACKS], s_valid[CK_PACKS], part[4];
    lk_load_splitters(H, L, s_splH, s_splL);
    for (uint32_t tile = tile0 + blockIdx.x; tile < tile1; tile += gridDim.x) {
        const uint32_t first = boff[tile];
        if (boff[tile + 1] == first) continue;  // (the same for every lane: a tile without records)
        const uint64_t t0 = (uint64_t)tile * CK_TILE;
        uint64_t codes[CK_RUN];
        uint32_t cnt = 0, mask = 0;
        ck_lane_windows(bases, n_buf, n_win, t0, aligned, s.k, s_codes, s_valid, [&](uint32_t j, uint64_t a) {
            const uint32_t before = cnt;
            lk_window_hits(a, s, H, s_splH, L, s_splL, [&](uint32_t, uint32_t, uint32_t) { cnt++; });
            codes[j] = a;
            if (cnt != before) mask |= 1u << j;
        });
        uint32_t carry = first;
        uint32_t at = block_scan_excl(cnt, carry, part);
        if (cnt && (uint64_t)at + cnt > win_lo && at < (uint64_t)win_lo + cap) {
#pragma unroll
            for (uint32_t j = 0; j < CK_RUN; j++) {
                if (!(mask >> j & 1u)) continue;
                const uint64_t pos = pos0 + t0 + (uint64_t)threadIdx.x * CK_RUN + j;
                lk_window_hits(codes[j], s, H, s_splH, L, s_splL, [&](uint32_t id, uint32_t h, uint32_t off) {
                    const uint32_t slot = at++;
                    if (slot >= win_lo && slot - win_lo < cap)
                        rec[slot - win_lo] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), id >> 1, (id & 1u) | (h << 8) | (off << 16));
                });
            }
        }
        __syncthreads();  // the tile's LDS words are written again in the next turn
    }
}

bool lk_list_ok(const LocateList& l) {
    if (l.n == 0) return l.ns == 0;
    return l.spl && l.keys && l.codes && l.ids && l.B >= 1 && l.ns == (l.n + l.B - 1) / l.B && l.ns <= LOCATE_SPLITTERS;
}

bool lk_shape_ok(uint64_t n_win, uint32_t k, uint32_t d, const LocateList& H, const LocateList& L, LkShape& s) {
    if (k < 1 || k > 31 || d > 1 || (d == 1 && k < 2) || n_win > LOCATE_MAX_PIECE || !lk_list_ok(H) || !lk_list_ok(L) || (d == 0 && L.n)) return false;
    s = LkShape{k, d, (k + 1) / 2, k / 2};
    return true;
}

uint32_t lk_tiles(uint64_t n_win) { return (uint32_t)((n_win + CK_TILE - 1) / CK_TILE); }

}  // namespace

uint32_t locate_tiles(uint64_t n_win) { return lk_tiles(n_win); }

hipError_t launch_locate_count(const uint8_t* bases, uint64_t n_buf, uint64_t n_win, uint32_t kmer_len, uint32_t mismatches, const LocateList& H,
                               const LocateList& L, uint32_t* bcnt, uint32_t* boff, unsigned long long* windows, hipStream_t st) {
    LkShape s;
    if (!lk_shape_ok(n_win, kmer_len, mismatches, H, L, s) || n_win > n_buf) return hipErrorInvalidValue;
    const uint32_t tiles = lk_tiles(n_win);
    if (!tiles) return hipSuccess;
    const int aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;
    hipLaunchKernelGGL(lk_count_kernel, dim3(std::min<uint32_t>(tiles, 2048)), dim3(CK_BLOCK), 0, st, bases, n_buf, n_win, s, H, L, aligned, tiles, bcnt,
                       windows);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_block_offsets(bcnt, tiles, boff, st);
}

hipError_t launch_locate_write(const uint8_t* bases, uint64_t n_buf, uint64_t n_win, uint32_t kmer_len, uint32_t mismatches, const LocateList& H,
                               const LocateList& L, const uint32_t* boff, uint32_t tile0, uint32_t tile1, uint32_t win_lo, uint32_t cap, uint64_t pos0,
                               LocateRecord* rec, hipStream_t st) {
    LkShape s;
    if (tile1 <= tile0 || !cap) return hipSuccess;
    if (!lk_shape_ok(n_win, kmer_len, mismatches, H, L, s) || n_win > n_buf || tile1 > lk_tiles(n_win)) return hipErrorInvalidValue;
    const int aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;
    hipLaunchKernelGGL(lk_write_kernel, dim3(std::min<uint32_t>(tile1 - tile0, 2048)), dim3(CK_BLOCK), 0, st, bases, n_buf, n_win, s, H, L, aligned, tile0,
                       tile1, boff, win_lo, cap, pos0, reinterpret_cast<uint4*>(rec));
    return hipGetLastError();
}

}  // namespace kgwas
