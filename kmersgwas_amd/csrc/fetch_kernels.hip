// fetch_kernels.hip — device side of fetch_reads (fetch.cpp): the reads of a resident piece of a read stream that
// hold at least min_hits windows spelling a query k-mer or its reverse complement.
//
// A piece is whole reads, each ended by '\n'. The windows are count_kernels.hip's (kmer_windows.h): a workgroup of 256 lanes takes
// a tile of 4096 positions, a lane rolls the codes of its 16 windows out of 48 packed positions; a newline is no base, so no window
// crosses a read's end. The queries are ONE sorted list of their canonical codes (kernels.h, LocateList with codes == keys), its
// splitters in LDS (sorted_search.h); ids[i] = query << 1 | (the canonical code is the reverse complement of the query as spelled).
// A window canonicalises its code and searches once. Ahead of the search an optional presence bitmap of 2^18 bits, built on the
// device from the list and held in LDS, turns most windows away.
//   mark    every lane stores the 16-bit hit mask of its windows: marks[] is a plain bitmap over the piece's positions, written
//           without atomics. Each hit adds 1 to kmer_windows[query]. The tile's newlines are counted for the next step.
//   starts  the scan of the tiles' newline counts numbers the newlines: starts[r] is the first byte of read r of the piece, read r
//           is the bytes [starts[r], starts[r + 1] - 1) and its windows start in [starts[r], starts[r + 1] - k).
//   reduce  one lane per read: the popcount of the read's bit range is n_hits, its first set bit first_pos. Kept reads (n_hits >=
//           min_hits) leave the way ld_kernels.hip's proxy records do: count per block of 256 reads, scan, write - in read order,
//           the same bytes in every run. A kept read looks its first hit window up once more, from the bases, for kmer and strand.
//           The write kernel numbers a block's records from boff[block] and stores those of the window [win_lo, win_lo + cap) to
//           rec[number - win_lo]: no store is made past rec[cap - 1].
// A lane walks its read's words however long the read is: reads of sequencing length (a few words) are what this is shaped for.
#include "block_prims.h"
#include "kernels.h"
#include "kmer_windows.h"
#include "sorted_search.h"

namespace kgwas {

namespace {

// the bit of a canonical code in the presence bitmap: the top FETCH_FILTER_BITS bits of its product with a fixed odd constant
__device__ __forceinline__ uint32_t fr_filter_bit(uint64_t c) { return (uint32_t)((c * 0x9E3779B97F4A7C15ull) >> (64 - FETCH_FILTER_BITS)); }

// Does the window with code a spell a query? id = query << 1 | flag, strand 0: as the query is spelled.
template <bool PRE>
__device__ __forceinline__ bool fr_lookup(uint64_t a, uint32_t k, const LocateList& Q, const uint64_t* spl, const uint32_t* bits, uint32_t& id,
                                          uint32_t& strand) {
    const uint64_t r = ck_revcomp(a, k), c = a < r ? a : r;
    if (PRE) {
        const uint32_t h = fr_filter_bit(c);
        if (!(bits[h >> 5] >> (h & 31u) & 1u)) return false;
    }
    const uint64_t i = fk_list_bound<false>(spl, Q.ns, Q.keys, Q.n, Q.B, c);
    if (i >= Q.n || Q.keys[i] != c) return false;
    id = Q.ids[i];
    strand = (uint32_t)(a != c) ^ (id & 1u);
    return true;
}

// bit j: the byte at p + j < n is a newline (16 positions from p on)
__device__ __forceinline__ uint32_t fr_newlines(const uint8_t* bases, uint64_t n, uint64_t p, bool aligned) {
    uint32_t m = 0;
    if (p + 16 <= n && aligned) {
        const uint4 v = *reinterpret_cast<const uint4*>(bases + p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) m |= (uint32_t)(((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == '\n') << i;
    } else if (p < n) {
        const uint32_t c = (uint32_t)min((uint64_t)16, n - p);
        for (uint32_t i = 0; i < c; i++) m |= (uint32_t)(bases[p + i] == '\n') << i;
    }
    return m;
}

__global__ void __launch_bounds__(256) fr_filter_kernel(LocateList Q, uint32_t* filter) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < Q.n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t h = fr_filter_bit(Q.keys[i]);
        atomicOr(&filter[h >> 5], 1u << (h & 31u));
    }
}

template <bool PRE>
__global__ void __launch_bounds__(CK_BLOCK) fr_mark_kernel(const uint8_t* __restrict__ bases, uint64_t n, uint32_t k, LocateList Q,
                                                           const uint32_t* __restrict__ filter, int aligned, uint32_t n_tiles, uint16_t* marks,
                                                           uint32_t* nlcnt, unsigned long long* kmer_windows, unsigned long long* windows) {
    __shared__ uint64_t s_spl[LOCATE_SPLITTERS];
    __shared__ uint32_t s_bits[PRE ? FETCH_FILTER_WORDS : 1];
    __shared__ uint32_t s_codes[CK_PACKS], s_valid[CK_PACKS], red[8];
    for (uint32_t i = threadIdx.x; i < Q.ns; i += CK_BLOCK) s_spl[i] = Q.spl[i];
    if (PRE)
        for (uint32_t i = threadIdx.x; i < FETCH_FILTER_WORDS; i += CK_BLOCK) s_bits[i] = filter[i];
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = (uint64_t)tile * CK_TILE;
        uint32_t mask = 0;
        uint32_t v[2];
        v[1] = ck_lane_windows(bases, n, n, t0, aligned, k, s_codes, s_valid, [&](uint32_t j, uint64_t a) {
            uint32_t id, strand;
            if (fr_lookup<PRE>(a, k, Q, s_spl, s_bits, id, strand)) {
                mask |= 1u << j;
                atomicAdd(&kmer_windows[id >> 1], 1ull);
            }
        });
        marks[(uint64_t)tile * CK_BLOCK + threadIdx.x] = (uint16_t)mask;
        v[0] = (uint32_t)__popc(fr_newlines(bases, n, t0 + (uint64_t)threadIdx.x * CK_RUN, aligned));
        block_sum(v, red);
        if (threadIdx.x == 0) {
            nlcnt[tile] = v[0];
            if (v[1]) atomicAdd(windows, (unsigned long long)v[1]);
        }
        __syncthreads();  // the tile's LDS words are written again in the next turn
    }
}

// starts[0] = 0; starts[r + 1] = the position behind the piece's r-th newline, for r < n_reads
__global__ void __launch_bounds__(CK_BLOCK) fr_starts_kernel(const uint8_t* __restrict__ bases, uint64_t n, int aligned, uint32_t n_tiles,
                                                             const uint32_t* nloff, uint32_t n_reads, uint32_t* starts) {
    __shared__ uint32_t part[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t p0 = (uint64_t)tile * CK_TILE + (uint64_t)threadIdx.x * CK_RUN;
        uint32_t m = fr_newlines(bases, n, p0, aligned);
        uint32_t carry = nloff[tile];
        uint32_t at = block_scan_excl((uint32_t)__popc(m), carry, part);
        for (; m; m &= m - 1u, at++)
            if (at < n_reads) starts[at + 1] = (uint32_t)(p0 + (uint32_t)(__ffs((int)m) - 1) + 1u);
        __syncthreads();  // part is written again in the next turn
    }
}

// Read r of the piece: its hit windows and the first of them (a position of the piece). words: the 32-bit words of marks[].
__device__ __forceinline__ uint32_t fr_read_hits(const uint32_t* __restrict__ words, const uint32_t* __restrict__ starts, uint64_t n, uint32_t r,
                                                 uint32_t k, uint32_t& first) {
    const uint32_t lo = starts[r], next = starts[r + 1];
    first = 0;
    if (next > n || next < lo + k + 1u) return 0;  // (fewer than k bytes ahead of the newline)
    const uint32_t hi = next - k;      // windows start in [lo, hi)
    uint32_t n_hits = 0;
    for (uint32_t w = lo >> 5; w <= (hi - 1u) >> 5; w++) {
        uint32_t x = words[w];
        if (w == lo >> 5) x &= 0xFFFFFFFFu << (lo & 31u);
        if (w == (hi - 1u) >> 5) x &= 0xFFFFFFFFu >> (31u - ((hi - 1u) & 31u));
        if (x && !n_hits) first = w * 32u + (uint32_t)(__ffs((int)x) - 1);
        n_hits += (uint32_t)__popc(x);
    }
    return n_hits;
}

__global__ void __launch_bounds__(256) fr_count_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ starts, uint64_t n,
                                                       uint32_t n_reads, uint32_t k, uint32_t min_hits, uint32_t* bcnt) {
    __shared__ uint32_t red[4];
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    uint32_t first;
    const uint32_t kept = r < n_reads && fr_read_hits(words, starts, n, r, k, first) >= min_hits;
    const uint32_t total = block_sum(kept, red);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

// the records numbered [win_lo, win_lo + cap) among those of the read blocks from blk0 on, to rec[number - win_lo]
__global__ void __launch_bounds__(256) fr_write_kernel(const uint8_t* __restrict__ bases, uint64_t n, const uint32_t* __restrict__ words,
                                                       const uint32_t* __restrict__ starts, uint32_t n_reads, uint32_t k, uint32_t min_hits,
                                                       LocateList Q, const uint32_t* boff, uint32_t blk0, uint32_t win_lo, uint32_t cap,
                                                       uint64_t read0, FetchRecord* rec) {
    __shared__ uint64_t s_spl[LOCATE_SPLITTERS];
    __shared__ uint32_t part[4];
    const uint32_t blk = blk0 + blockIdx.x;
    if (boff[blk + 1] == boff[blk]) return;  // (the same for every lane: a block without records)
    for (uint32_t i = threadIdx.x; i < Q.ns; i += 256u) s_spl[i] = Q.spl[i];
    const uint32_t r = blk * 256u + threadIdx.x;
    uint32_t first = 0, n_hits = 0;
    if (r < n_reads) n_hits = fr_read_hits(words, starts, n, r, k, first);
    const uint32_t kept = r < n_reads && n_hits >= min_hits;
    uint32_t carry = boff[blk];
    const uint32_t slot = block_scan_excl(kept, carry, part);  // (its barrier also ends the splitters' load)
    if (!kept || slot < win_lo || slot - win_lo >= cap) return;
    uint32_t id = 0xFFFFFFFFu, strand = 0;  // (a window that is no hit after all: the host refuses the record)
    if ((uint64_t)first + k <= n) {
        uint64_t a = 0;
        for (uint32_t i = 0; i < k; i++) a = a << 2 | (ck_code(bases[first + i]) & 3u);
        if (!fr_lookup<false>(a, k, Q, s_spl, nullptr, id, strand)) id = 0xFFFFFFFFu;
    }
    FetchRecord out{};
    out.read = read0 + r, out.n_hits = n_hits, out.first_pos = first - starts[r];
    out.kmer = id == 0xFFFFFFFFu ? id : id >> 1, out.strand = (uint8_t)strand;
    rec[slot - win_lo] = out;
}

bool fr_shape_ok(uint64_t n, uint32_t k, const LocateList& Q) {
    return k >= 1 && k <= 31 && n <= LOCATE_MAX_PIECE && Q.n >= 1 && Q.spl && Q.keys && Q.codes == Q.keys && Q.ids && Q.B >= 1 &&
           Q.ns == (Q.n + Q.B - 1) / Q.B && Q.ns <= LOCATE_SPLITTERS;
}

}  // namespace

hipError_t launch_fetch_filter(const LocateList& Q, uint32_t* filter, hipStream_t st) {
    if (!fr_shape_ok(0, 1, Q) || !filter) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(filter, 0, FETCH_FILTER_WORDS * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fr_filter_kernel, dim3((uint32_t)std::min<uint64_t>((Q.n + 255u) / 256u, 1024)), dim3(256), 0, st, Q, filter);
    return hipGetLastError();
}

hipError_t launch_fetch_mark(const uint8_t* bases, uint64_t n, uint32_t kmer_len, const LocateList& Q, const uint32_t* filter, uint16_t* marks,
                             uint32_t* nlcnt, uint32_t* nloff, unsigned long long* kmer_windows, unsigned long long* windows, hipStream_t st) {
    if (!fr_shape_ok(n, kmer_len, Q) || !bases || !marks || !nlcnt || !nloff || !kmer_windows || !windows) return hipErrorInvalidValue;
    const uint32_t tiles = locate_tiles(n);
    if (!tiles) return hipSuccess;
    const int aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;
    const dim3 grid(std::min<uint32_t>(tiles, 2048));
    if (filter)
        hipLaunchKernelGGL(fr_mark_kernel<true>, grid, dim3(CK_BLOCK), 0, st, bases, n, kmer_len, Q, filter, aligned, tiles, marks, nlcnt, kmer_windows,
                           windows);
    else
        hipLaunchKernelGGL(fr_mark_kernel<false>, grid, dim3(CK_BLOCK), 0, st, bases, n, kmer_len, Q, filter, aligned, tiles, marks, nlcnt, kmer_windows,
                           windows);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_block_offsets(nlcnt, tiles, nloff, st);
}

hipError_t launch_fetch_count(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t min_hits, const uint16_t* marks, const uint32_t* nloff,
                              uint32_t n_reads, uint32_t* starts, uint32_t* bcnt, uint32_t* boff, hipStream_t st) {
    if (kmer_len < 1 || kmer_len > 31 || !min_hits || n > LOCATE_MAX_PIECE || n_reads > n || !bases || !marks || !nloff || !starts || !bcnt || !boff)
        return hipErrorInvalidValue;
    const uint32_t tiles = locate_tiles(n);
    if (!tiles || !n_reads) return hipSuccess;
    const int aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;
    hipLaunchKernelGGL(fr_starts_kernel, dim3(std::min<uint32_t>(tiles, 2048)), dim3(CK_BLOCK), 0, st, bases, n, aligned, tiles, nloff, n_reads, starts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t blocks = fetch_read_blocks(n_reads);
    hipLaunchKernelGGL(fr_count_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(marks), starts, n, n_reads, kmer_len,
                       min_hits, bcnt);
    e = hipGetLastError();
    return e != hipSuccess ? e : launch_block_offsets(bcnt, blocks, boff, st);
}

hipError_t launch_fetch_write(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t min_hits, const LocateList& Q, const uint16_t* marks,
                              const uint32_t* starts, uint32_t n_reads, const uint32_t* boff, uint32_t blk0, uint32_t blk1, uint32_t win_lo, uint32_t cap,
                              uint64_t read0, FetchRecord* rec, hipStream_t st) {
    if (blk1 <= blk0 || !cap) return hipSuccess;
    if (!fr_shape_ok(n, kmer_len, Q) || !min_hits || n_reads > n || blk1 > fetch_read_blocks(n_reads) || !bases || !marks || !starts || !boff || !rec)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fr_write_kernel, dim3(blk1 - blk0), dim3(256), 0, st, bases, n, reinterpret_cast<const uint32_t*>(marks), starts, n_reads, kmer_len,
                       min_hits, Q, boff, blk0, win_lo, cap, read0, rec);
    return hipGetLastError();
}

}  // namespace kgwas
