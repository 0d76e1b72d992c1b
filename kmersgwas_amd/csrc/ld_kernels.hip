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
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 8; y++) acc[x][y] = (kin_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += 4u) {  // n_chunks is a multiple of 4
        const uint4* base = P + (uint64_t)(c0 + kg) * N_pad;
        uint4 wA[4], wB[8];
#pragma unroll
        for (int x = 0; x < 4; x++) wA[x] = base[a0 + 16u * x + m];
#pragma unroll
        for (int y = 0; y < 8; y++) wB[y] = base[b0 + 16u * y + m];
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

hipError_t launch_ld_prep(const uint64_t* rows, uint64_t stride_w, uint64_t W, uint64_t N, uint32_t n, uint32_t n_chunks, uint64_t N_pad,
                          uint32_t tm, void* P, uint32_t* n1, uint32_t* pq, uint64_t* tq, hipStream_t st) {
    const uint64_t total = (uint64_t)n_chunks * N_pad;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(ld_prep_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, st, rows, stride_w, W, N, n, n_chunks, N_pad,
                       tm, (uint4*)P, n1, pq, tq);
    return hipGetLastError();
}

hipError_t launch_ld_link(const void* P, const uint32_t* n1, const uint32_t* pq, const uint64_t* tq, uint64_t N, uint64_t N_pad, uint32_t n,
                          uint32_t n_chunks, uint64_t row0, uint64_t n_rows, uint32_t* out, uint64_t pitch_dw, bool popcount, hipStream_t st) {
    if (!n_rows) return hipSuccess;
    // what the kernels assume and do not check: whole tiles of padded operands, and a pitch that holds every tile's 16-byte stores
    if (N_pad % 128u || n_chunks % 4u || row0 % 64u || row0 + (n_rows + 63u) / 64u * 64u > N_pad || pitch_dw % 4u || pitch_dw * 32u < N_pad)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(N_pad / 128u), (uint32_t)((n_rows + 63u) / 64u));
    if (popcount)
        hipLaunchKernelGGL(ld_link_popc_kernel, grid, dim3(64), 0, st, (const uint4*)P, n1, pq, tq, N, N_pad, n, n_chunks, row0, out, pitch_dw);
    else
        hipLaunchKernelGGL(ld_link_kernel, grid, dim3(64), 0, st, (const uint4*)P, n1, pq, tq, N, N_pad, n, n_chunks, row0, out, pitch_dw);
    return hipGetLastError();
}

}  // namespace kgwas
