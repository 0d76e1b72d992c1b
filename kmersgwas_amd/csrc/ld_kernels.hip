// ld_kernels.hip — clump_kmers' hot path: which pairs of presence/absence rows have r^2 >= t, exactly.
//
// For rows a, b over n accessions with presence counts ca, cb and n11 accessions in common,
//     r^2 = (n n11 - ca cb)^2 / (ca (n - ca) cb (n - cb)),
// a ratio of integers: the pair is linked iff the denominator is positive and num * 10^6 >= tm * den with tm the threshold in
// millionths - decided in 128-bit integers, no rounding anywhere. Two kernels:
//   ld_prep_kernel : the rows as they arrive (bit i of a row = accession i) into chunks of 128 accessions, chunk-major
//                    P[chunk][row] (one 16-byte load per lane and operand), bits at or past n masked, rows and chunks padded
//                    with zeros to whole tiles so that the Gram kernel loads without a bound; per row its count n1,
//                    pq = n1 (n - n1) and tq = tm pq.
//   ld_link_kernel : n11 = R R^t on the block-scaled FP4 MFMA (fp4_bits.h: the kinship kernel's operand trick, here with
//                    M and N k-mers and the K dimension accessions - the rows are the operands as they stand, nothing is
//                    transposed), then the predicate per accumulator element and 32 predicates per dword by ballots. A wave
//                    owns 64 rows a x 128 rows b: 32 accumulators (128 registers), 12 operand expansions (4 lane-ops each)
//                    per 32 MFMAs. The matrix of counts never leaves the registers; what is written is one bit per pair.
// proxy_kmers adds the rectangular form, few resident leads against a piece of table rows (ld_rect_kernel, the same
// MFMA loop and predicate), and the compaction of its bits into records in a fixed order (ld_proxy_count / scan / write kernels).
#include "block_prims.h"
#include "fp4_bits.h"
#include "kernels.h"

namespace kgwas {

namespace {

// linked(a, b) from the integers: d = n n11 - ca cb (|d| <= 2^26; every factor is below 2^24, so the two products are 24-bit
// multiplies), num = d^2 < 2^52, den = pa pb <= 2^48 with pa = ca (n - ca); tqb = tm pb < 2^44 comes ready from ld_prep_kernel.
// num * 10^6 >= pa * tqb is a compare of two products of up to 72 bits. No branch: the wave's lanes all do the same work.
__device__ __forceinline__ bool ld_linked(uint32_t n, uint32_t n11, uint32_t ca, uint32_t cb, uint32_t pa, uint64_t tqb) {
    const int32_t d = (int32_t)__umul24(n, n11) - (int32_t)__umul24(ca, cb);
    const uint32_t e = (uint32_t)(d < 0 ? -d : d);
    const uint64_t num = (uint64_t)e * e;
    const unsigned __int128 lhs = (unsigned __int128)num * 1000000u, rhs = (unsigned __int128)tqb * pa;
    return (pa != 0u) & (tqb != 0ull) & (lhs >= rhs);
}

// n11 of the wave's tile, 64 rows a of [a0, +64) x 128 rows b of [b0, +128), on the matrix cores: acc[x][y][jj] of lane (m, kg) is
// n11 of a = a0 + 16 x + 4 kg + jj, b = b0 + 16 y + m. PA[chunk][padA] and PB[chunk][padB] are ld_prep_kernel's operand arrays (one
// array in the square case). Shared by ld_link_kernel and ld_rect_kernel.
__device__ __forceinline__ void ld_tile_counts(const uint4* PA, uint64_t padA, uint64_t a0, const uint4* PB, uint64_t padB, uint64_t b0,
                                               uint32_t n_chunks, uint32_t m, uint32_t kg, kin_f32x4 (&acc)[4][8]) {
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 8; y++) acc[x][y] = (kin_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += 4u) {  // n_chunks is a multiple of 4
        const uint4 *baseA = PA + (uint64_t)(c0 + kg) * padA, *baseB = PB + (uint64_t)(c0 + kg) * padB;
        uint4 wA[4], wB[8];
#pragma unroll
        for (int x = 0; x < 4; x++) wA[x] = baseA[a0 + 16u * x + m];
#pragma unroll
        for (int y = 0; y < 8; y++) wB[y] = baseB[b0 + 16u * y + m];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            kin_i32x8 A[4];
#pragma unroll
            for (int x = 0; x < 4; x++) A[x] = kin_expand_step(wA[x], j);
#pragma unroll
            for (int y = 0; y < 8; y++) {
                const kin_i32x8 B = kin_expand_step(wB[y], j);
                // both operands FP4 (cbsz = blgp = 4); block scales 2^1, 2^0, 2^-1, 2^-1 for j = 0..3 on both sides
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (j == 0) acc[x][y] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[x], B, acc[x][y], 4, 4, 0, (int)0x80808080, 0, (int)0x80808080);
                    if (j == 1) acc[x][y] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[x], B, acc[x][y], 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
                    if (j >= 2) acc[x][y] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[x], B, acc[x][y], 4, 4, 0, 0x7E7E7E7E, 0, 0x7E7E7E7E);
                }
            }
        }
    }
}

}  // namespace

// One thread per (row, chunk) of the padded operand array; the threads of chunk 0 also count their row.
__global__ void __launch_bounds__(256) ld_prep_kernel(const uint64_t* rows, uint64_t stride_w, uint64_t W, uint64_t N, uint32_t n,
                                                      uint32_t n_chunks, uint64_t N_pad, uint32_t tm, uint4* P, uint32_t* n1, uint32_t* pq, uint64_t* tq) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)n_chunks * N_pad) return;
    const uint32_t c = (uint32_t)(i / N_pad);
    const uint64_t r = i - (uint64_t)c * N_pad;
    auto word = [&](uint64_t w) -> uint64_t {  // word w of row r, bits at or past n cleared
        if (r >= N || w >= W || 64u * w >= n) return 0ull;
        uint64_t x = rows[r * stride_w + w];
        if (64u * w + 64u > n) x &= (1ull << (n - 64u * w)) - 1ull;
        return x;
    };
    const uint64_t lo = word(2ull * c), hi = word(2ull * c + 1ull);
    P[i] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    if (c == 0) {
        uint32_t cnt = 0;
        for (uint64_t w = 0; w < W && 64u * w < n; w++) cnt += (uint32_t)__popcll(word(w));
        n1[r] = cnt;
        pq[r] = cnt * (n - cnt);  // <= 2^24 with n <= 8192
        tq[r] = (uint64_t)tm * (cnt * (n - cnt));
    }
}

// Rows a of [row0 + 64 blockIdx.y, +64) against rows b of [128 blockIdx.x, +128): the 64 x 4 dwords of the link matrix they
// cover go to out[(a - row0) * pitch_dw + b / 32], zero on and below the diagonal and past N. One wave per block.
// MFMA k index <-> accessions: per round of 512 accessions lane (m, kg) holds chunk 4 round + kg of its rows and step j = 0..3
// takes bit j of each of its nibbles (kin_expand_step): A and B use the same map, so an accession meets itself.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) ld_link_kernel(const uint4* P, const uint32_t* n1, const uint32_t* pq, const uint64_t* tq, uint64_t N, uint64_t N_pad,
                                                     uint32_t n, uint32_t n_chunks, uint64_t row0, uint32_t* out,
                                                     uint64_t pitch_dw) {
    const uint32_t lane = threadIdx.x & 63u, m = lane & 15u, kg = lane >> 4;
    const uint64_t a0 = row0 + 64ull * blockIdx.y, b0 = 128ull * blockIdx.x;
    // the lane's store: row 16 (m / 4) + 4 kg + (m % 4) of the tile, four dwords
    const uint32_t my_row = 16u * (m >> 2) + 4u * kg + (m & 3u);
    uint4* dst = reinterpret_cast<uint4*>(out + ((a0 - row0) + my_row) * pitch_dw + b0 / 32u);
    if (b0 + 127u <= a0) {  // wholly on or below the diagonal (wave-uniform)
        *dst = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    kin_f32x4 acc[4][8];
    ld_tile_counts(P, N_pad, a0, P, N_pad, b0, n_chunks, m, kg, acc);
    // acc[x][y][jj] of lane (m, kg) is n11 of a = a0 + 16 x + 4 kg + jj, b = b0 + 16 y + m. A ballot over the wave's predicates
    // for one (x, y, jj) holds, in its bits 16 kg' ..+15, the 16 columns of sub-tile y for row 16 x + 4 kg' + jj: the lane whose
    // store row that is (m = 4 x + jj, kg = kg') takes them into half (y & 1) of its dword y / 2.
    uint32_t cb[8];
    uint64_t tqb[8];
#pragma unroll
    for (int y = 0; y < 8; y++) {
        cb[y] = n1[b0 + 16u * y + m];
        tqb[y] = tq[b0 + 16u * y + m];
    }
    const uint32_t a32 = (uint32_t)a0 + 4u * kg, b32 = (uint32_t)b0 + m, N32 = (uint32_t)N;  // (indices are below 2^20 + 128)
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int x = 0; x < 4; x++) {
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const uint64_t a = a0 + 16u * x + 4u * kg + jj;
            const uint32_t ca = n1[a], pa = pq[a];
            const bool mine = m == (uint32_t)(4 * x + jj);
#pragma unroll
            for (int y = 0; y < 8; y++) {
                const uint32_t ai = a32 + 16u * x + jj, bi = b32 + 16u * y;
                const bool link = (bi > ai) & (bi < N32) & ld_linked(n, (uint32_t)acc[x][y][jj], ca, cb[y], pa, tqb[y]);
                const uint64_t bal = __ballot(link);
                if (mine) v[y >> 1] |= ((uint32_t)(bal >> (16u * kg)) & 0xFFFFu) << (16u * (y & 1));
            }
            __builtin_amdgcn_sched_barrier(0);  // one row of predicates at a time: the ballots' scalar registers stay few
        }
    }
    *dst = make_uint4(v[0], v[1], v[2], v[3]);
}

// The guarded ablation: the same tile and output with n11 from popcount(AND) on the vector ALU instead of the matrix cores.
// Lane (m, kg) computes the tile's elements one at a time; it exists for the comparison in DESIGN.md 4.13 and for the tests'
// second opinion (KGWAS_LD_POPCOUNT=1), not as a path of its own.
__global__ void __launch_bounds__(64) ld_link_popc_kernel(const uint4* P, const uint32_t* n1, const uint32_t* pq, const uint64_t* tq, uint64_t N, uint64_t N_pad,
                                                          uint32_t n, uint32_t n_chunks, uint64_t row0, uint32_t* out,
                                                          uint64_t pitch_dw) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t a0 = row0 + 64ull * blockIdx.y, b0 = 128ull * blockIdx.x;
    const uint64_t a = a0 + lane;  // the lane's row: its four dwords, bit by bit
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (b0 + 127u > a0) {
        const uint32_t ca = n1[a], pa = pq[a];
        for (uint32_t k = 0; k < 128u; k++) {
            const uint64_t b = b0 + k;  // (wave-uniform: the loads of row b are broadcasts)
            uint32_t n11 = 0;
            for (uint32_t c = 0; c < n_chunks; c++) {
                const uint4 x = P[(uint64_t)c * N_pad + a], y = P[(uint64_t)c * N_pad + b];
                n11 += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
            }
            if (b > a && b < N && ld_linked(n, n11, ca, n1[b], pa, tq[b])) v[k >> 5] |= 1u << (k & 31u);
        }
    }
    *reinterpret_cast<uint4*>(out + ((a0 - row0) + lane) * pitch_dw + b0 / 32u) = make_uint4(v[0], v[1], v[2], v[3]);
}

// ---- proxy_kmers: few leads against a piece of table rows -------------------------------------------------------
// The rectangular form of ld_link_kernel: leads a of [64 blockIdx.y, +64) (the A operands, resident for the whole pass) against the
// piece's rows b of [128 blockIdx.x, +128), each side with its own operand array and n1, pq, tq. There is no diagonal rule: every
// pair is tested. The bits are stored ROW-major, out[b * pitch_q + a / 64] bit a % 64, so that the compaction below reads a row's
// leads in ascending order from consecutive words: lane (m, kg) holds the predicates of 16 leads (x, jj) for each of its 8 rows b
// (y), so a row's 64 bits are the OR of four lanes' 16 (two shuffles) - no ballot. Pad leads and pad rows have n1 = 0 and link to
// nothing; the bounds are tested as well. Every word of out[R_pad][pitch_q] under the grid is written.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
ld_rect_kernel(const uint4* PA, const uint32_t* n1A, const uint32_t* pqA, uint32_t L, uint64_t L_pad, const uint4* PB, const uint32_t* n1B,
               const uint64_t* tqB, uint32_t R, uint64_t R_pad, uint32_t n, uint32_t n_chunks, uint64_t* out, uint64_t pitch_q) {
    const uint32_t lane = threadIdx.x & 63u, m = lane & 15u, kg = lane >> 4;
    const uint64_t a0 = 64ull * blockIdx.y, b0 = 128ull * blockIdx.x;
    kin_f32x4 acc[4][8];
    ld_tile_counts(PA, L_pad, a0, PB, R_pad, b0, n_chunks, m, kg, acc);
    uint32_t cb[8];
    uint64_t tqb[8], w[8];
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const uint32_t b = (uint32_t)b0 + 16u * y + m;
        cb[y] = n1B[b];
        tqb[y] = b < R ? tqB[b] : 0ull;  // (a zero tq links to nothing)
        w[y] = 0ull;
    }
#pragma unroll
    for (int x = 0; x < 4; x++) {
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const uint32_t a = (uint32_t)a0 + 16u * x + 4u * kg + jj;
            const uint32_t ca = n1A[a], pa = a < L ? pqA[a] : 0u;  // (a zero pq links to nothing)
#pragma unroll
            for (int y = 0; y < 8; y++)
                w[y] |= (uint64_t)ld_linked(n, (uint32_t)acc[x][y][jj], ca, cb[y], pa, tqb[y]) << (16 * x + jj);
        }
    }
#pragma unroll
    for (int y = 0; y < 8; y++) {
        uint64_t v = w[y] << (4u * kg);  // bit 16 x + 4 kg + jj: the lead's place in the tile
        v |= __shfl_xor(v, 16);
        v |= __shfl_xor(v, 32);
        if (kg == (uint32_t)(y & 3)) out[(b0 + 16u * y + m) * pitch_q + blockIdx.y] = v;
    }
}

// The guarded ablation of ld_rect_kernel (KGWAS_LD_POPCOUNT=1): the same tile and words with n11 from popcount(AND) on the vector
// ALU. Lane l takes rows b0 + l and b0 + 64 + l; the lead is wave-uniform, its loads are broadcasts.
__global__ void __launch_bounds__(64) ld_rect_popc_kernel(const uint4* PA, const uint32_t* n1A, const uint32_t* pqA, uint32_t L, uint64_t L_pad,
                                                          const uint4* PB, const uint32_t* n1B, const uint64_t* tqB, uint32_t R, uint64_t R_pad,
                                                          uint32_t n, uint32_t n_chunks, uint64_t* out, uint64_t pitch_q) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t a0 = 64ull * blockIdx.y, b0 = 128ull * blockIdx.x;
    for (uint32_t h = 0; h < 2u; h++) {
        const uint64_t b = b0 + 64u * h + lane;
        const uint32_t cb = n1B[b];
        const uint64_t tqb = b < R ? tqB[b] : 0ull;
        uint64_t v = 0ull;
        for (uint32_t k = 0; k < 64u; k++) {
            const uint64_t a = a0 + k;
            uint32_t n11 = 0;
            for (uint32_t c = 0; c < n_chunks; c++) {
                const uint4 x = PA[(uint64_t)c * L_pad + a], y = PB[(uint64_t)c * R_pad + b];
                n11 += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
            }
            if (a < L && ld_linked(n, n11, n1A[a], cb, pqA[a], tqb)) v |= 1ull << k;
        }
        out[b * pitch_q + blockIdx.y] = v;
    }
}

namespace {

// the linked leads of row r: the set bits of its pitch_q words
__device__ __forceinline__ uint32_t proxy_row_count(const uint64_t* bits, uint64_t pitch_q, uint32_t r, uint32_t R) {
    uint32_t cnt = 0;
    if (r < R)
        for (uint64_t q = 0; q < pitch_q; q++) cnt += (uint32_t)__popcll(bits[(uint64_t)r * pitch_q + q]);
    return cnt;
}

}  // namespace

// The sparse result in three launches, with the same records in the same places in every run. Records are numbered in (row, lead)
// order over the piece; a block is 256 consecutive rows.
//   count: bcnt[block] = the block's records
//   scan : boff[block] = the records before the block, boff[n_blocks] = the piece's total (one block walks the counts)
//   write: the records numbered [win_lo, win_lo + cap) go to rec[number - win_lo] - the host drains a piece with more records than
//          the buffer holds in several rounds, each over the blocks of rows its window meets. No store is made past rec[cap - 1].
__global__ void __launch_bounds__(256) ld_proxy_count_kernel(const uint64_t* bits, uint64_t pitch_q, uint32_t R, uint32_t* bcnt) {
    __shared__ uint32_t red[4];
    const uint32_t total = block_sum(proxy_row_count(bits, pitch_q, blockIdx.x * 256u + threadIdx.x, R), red);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) ld_proxy_scan_kernel(const uint32_t* bcnt, uint32_t n_blocks, uint32_t* boff) {
    __shared__ uint32_t part[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t o = block_scan_excl(i < n_blocks ? bcnt[i] : 0u, carry, part);
        if (i < n_blocks) boff[i] = o;
        __syncthreads();  // part is written again in the next turn
    }
    if (threadIdx.x == 0) boff[n_blocks] = carry;
}

// n11 of a record is popcount(AND) over the two rows' operand chunks (bits at or past n are already cleared there). kmers (may be
// null: 0) holds row r's k-mer word at kmers[r * kmer_stride]; row_base is the piece's first row.
__global__ void __launch_bounds__(256) ld_proxy_write_kernel(const uint64_t* bits, uint64_t pitch_q, uint32_t R, const uint32_t* boff, uint32_t blk0,
                                                             uint32_t win_lo, uint32_t cap, const uint4* PA, uint64_t L_pad, const uint4* PB,
                                                             uint64_t R_pad, uint32_t n_chunks, const uint32_t* n1B, const uint64_t* kmers,
                                                             uint64_t kmer_stride, uint64_t row_base, ProxyRecord* rec) {
    __shared__ uint32_t part[4];
    const uint32_t blk = blk0 + blockIdx.x, r = blk * 256u + threadIdx.x;
    const uint32_t cnt = proxy_row_count(bits, pitch_q, r, R);
    uint32_t carry = boff[blk];
    uint32_t at = block_scan_excl(cnt, carry, part);
    if (!cnt || (uint64_t)at + cnt <= win_lo || at >= (uint64_t)win_lo + cap) return;  // none of the row's records is in the window
    const uint64_t kmer = kmers ? kmers[(uint64_t)r * kmer_stride] : 0ull;
    const uint32_t n1 = n1B[r];
    for (uint64_t q = 0; q < pitch_q; q++) {
        uint64_t x = bits[(uint64_t)r * pitch_q + q];
        for (; x; x &= x - 1ull, at++) {
            if (at < win_lo || at - win_lo >= cap) continue;
            const uint32_t lead = (uint32_t)(64u * q) + (uint32_t)__ffsll((unsigned long long)x) - 1u;
            uint32_t n11 = 0;
            for (uint32_t c = 0; c < n_chunks; c++) {
                const uint4 u = PA[(uint64_t)c * L_pad + lead], v = PB[(uint64_t)c * R_pad + r];
                n11 += __popc(u.x & v.x) + __popc(u.y & v.y) + __popc(u.z & v.z) + __popc(u.w & v.w);
            }
            rec[at - win_lo] = ProxyRecord{row_base + r, kmer, lead, n1, n11, 0u};
        }
    }
}

hipError_t launch_ld_rect(const LdView& A, const LdView& B, uint32_t n, uint64_t* out, uint64_t pitch_q, bool popcount, hipStream_t st) {
    const uint64_t L = A.count, L_pad = A.pad, R = B.count, R_pad = B.pad;
    if (!R || !L) return hipSuccess;
    // what the kernels assume and do not check: whole tiles of padded operands and a pitch that holds every lead tile's word
    if (L_pad % 64u || R_pad % 128u || A.n_chunks % 4u || B.n_chunks != A.n_chunks || L > L_pad || R > R_pad || pitch_q * 64u < L_pad || L_pad > 4096u ||
        R_pad > (1ull << 20))
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(R_pad / 128u), (uint32_t)(L_pad / 64u));
    if (popcount)
        hipLaunchKernelGGL(ld_rect_popc_kernel, grid, dim3(64), 0, st, (const uint4*)A.P, (const uint32_t*)A.n1, (const uint32_t*)A.pq, (uint32_t)L, L_pad,
                           (const uint4*)B.P, (const uint32_t*)B.n1, (const uint64_t*)B.tq, (uint32_t)R, R_pad, n, A.n_chunks, out, pitch_q);
    else
        hipLaunchKernelGGL(ld_rect_kernel, grid, dim3(64), 0, st, (const uint4*)A.P, (const uint32_t*)A.n1, (const uint32_t*)A.pq, (uint32_t)L, L_pad,
                           (const uint4*)B.P, (const uint32_t*)B.n1, (const uint64_t*)B.tq, (uint32_t)R, R_pad, n, A.n_chunks, out, pitch_q);
    return hipGetLastError();
}

hipError_t launch_ld_proxy_count(const uint64_t* bits, uint64_t pitch_q, uint64_t R, uint32_t* bcnt, uint32_t* boff, hipStream_t st) {
    if (!R) return hipSuccess;
    if (R > (1ull << 20)) return hipErrorInvalidValue;
    const uint32_t n_blocks = (uint32_t)((R + 255u) / 256u);
    hipLaunchKernelGGL(ld_proxy_count_kernel, dim3(n_blocks), dim3(256), 0, st, bits, pitch_q, (uint32_t)R, bcnt);
    return launch_block_offsets(bcnt, n_blocks, boff, st);
}

hipError_t launch_block_offsets(const uint32_t* bcnt, uint32_t n_blocks, uint32_t* boff, hipStream_t st) {
    hipLaunchKernelGGL(ld_proxy_scan_kernel, dim3(1), dim3(256), 0, st, bcnt, n_blocks, boff);
    return hipGetLastError();
}

hipError_t launch_ld_proxy_write(const uint64_t* bits, uint64_t pitch_q, const uint32_t* boff, uint32_t blk0, uint32_t blk1, uint32_t win_lo,
                                 uint32_t cap, const LdView& A, const LdView& B, const uint64_t* kmers, uint64_t kmer_stride, uint64_t row_base,
                                 ProxyRecord* rec, hipStream_t st) {
    if (blk1 <= blk0 || !cap) return hipSuccess;
    if ((uint64_t)blk1 * 256u > (B.count + 255u) / 256u * 256u || A.n_chunks != B.n_chunks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ld_proxy_write_kernel, dim3(blk1 - blk0), dim3(256), 0, st, bits, pitch_q, (uint32_t)B.count, boff, blk0, win_lo, cap,
                       (const uint4*)A.P, A.pad, (const uint4*)B.P, B.pad, B.n_chunks, (const uint32_t*)B.n1, kmers, kmer_stride, row_base, rec);
    return hipGetLastError();
}

hipError_t launch_ld_prep(const uint64_t* rows, uint64_t stride_w, uint64_t W, uint32_t n, uint32_t tm, const LdView& ops, hipStream_t st) {
    const uint64_t total = (uint64_t)ops.n_chunks * ops.pad;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(ld_prep_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, st, rows, stride_w, W, ops.count, n, ops.n_chunks, ops.pad,
                       tm, (uint4*)ops.P, ops.n1, ops.pq, ops.tq);
    return hipGetLastError();
}

hipError_t launch_ld_link(const LdView& ops, uint32_t n, uint64_t row0, uint64_t n_rows, uint32_t* out, uint64_t pitch_dw, bool popcount,
                          hipStream_t st) {
    const uint64_t N = ops.count, N_pad = ops.pad;
    if (!n_rows) return hipSuccess;
    // what the kernels assume and do not check: whole tiles of padded operands, and a pitch that holds every tile's 16-byte stores
    if (N_pad % 128u || ops.n_chunks % 4u || row0 % 64u || row0 + (n_rows + 63u) / 64u * 64u > N_pad || pitch_dw % 4u || pitch_dw * 32u < N_pad)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(N_pad / 128u), (uint32_t)((n_rows + 63u) / 64u));
    if (popcount)
        hipLaunchKernelGGL(ld_link_popc_kernel, grid, dim3(64), 0, st, (const uint4*)ops.P, (const uint32_t*)ops.n1, (const uint32_t*)ops.pq,
                           (const uint64_t*)ops.tq, N, N_pad, n, ops.n_chunks, row0, out, pitch_dw);
    else
        hipLaunchKernelGGL(ld_link_kernel, grid, dim3(64), 0, st, (const uint4*)ops.P, (const uint32_t*)ops.n1, (const uint32_t*)ops.pq,
                           (const uint64_t*)ops.tq, N, N_pad, n, ops.n_chunks, row0, out, pitch_dw);
    return hipGetLastError();
}

}  // namespace kgwas
