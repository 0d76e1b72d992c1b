// snpkin_kernels.hip — device side of emma_kinship (src/emma_kinship.cpp).
//
// The reference adds, for every SNP with a called sample and every pair r > c of samples, two terms to K[r][c]
// (update_K, :46-53): a_r*a_c + (1-a_r)*(1-a_c), once with pass A's values and once with pass B's (:112-135). Each
// pair's sum is a sequential double sum in SNP order, so the SNP axis is never split or reordered: parallelism is over
// pairs only, and every term is evaluated as written, one IEEE rounding per operation (__dmul_rn / __dsub_rn /
// __dadd_rn, no FMA), so the sums are bit-identical to the reference's.
//
//   snpkin_prep_kernel      one block per SNP of a chunk: the counts of the SNP (integers, any order is exact), its
//                           missing-call values mA = n_alt / n_total and mB = (n_alt + n_het) / n_total with IEEE
//                           division, and every sample's (a, 1-a) for both passes into vals[snp][sample] (a row of
//                           snpkin_vals_stride(S) entries: the 8 past the last sample are zero, so a tile's rows are
//                           consecutive entries and need no clamp)
//   snpkin_accumulate_kernel one wave per tile of RW rows x 64 columns of the lower triangle: rows wave-uniform (their
//                           values are scalar loads of vals), columns one per lane (decoded from the .bed byte once
//                           per SNP). The RW accumulators of a lane stay in registers across the chunk's SNPs.
//
// A SNP without a called sample (n_total == 0) is skipped by the reference. Here its values are all zero (every one of
// its samples is missing and mA, mB are set to 0), so both of its terms are +0 and acc + 0 = acc exactly: the loop
// needs no branch, and the SNP is left out of the used-SNP count.
#include "kernels.h"

namespace kgwas {

namespace {

struct SnpVals {  // one sample of one SNP: (a, 1-a) of pass A, then of pass B
    double a, oa, b, ob;
};

__global__ void __launch_bounds__(256) snpkin_prep_kernel(const uint8_t* __restrict__ bed, uint32_t bytes_per_snp, uint32_t S,
                                                          uint32_t Sv, SnpVals* __restrict__ params, SnpVals* __restrict__ vals,
                                                          unsigned long long* __restrict__ n_used) {
    const uint32_t snp = blockIdx.x;
    const uint8_t* row = bed + (uint64_t)snp * bytes_per_snp;
    __shared__ uint32_t cnt[3];  // missing, het, alt
    __shared__ SnpVals miss;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n_miss = 0, n_het = 0, n_alt = 0;
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
        const uint32_t d = (row[s >> 2] >> (2u * (s & 3u))) & 3u;  // :121
        n_miss += d == 1u;
        n_het += d == 2u;
        n_alt += d == 3u;
    }
    atomicAdd(&cnt[0], n_miss);
    atomicAdd(&cnt[1], n_het);
    atomicAdd(&cnt[2], n_alt);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n_total = S - cnt[0];
        SnpVals m = {0.0, 0.0, 0.0, 0.0};
        if (n_total > 0) {
            const double tot = (double)n_total;
            m.a = __ddiv_rn((double)cnt[2], tot);                                    // maf = n_var_allele / n_total (:129)
            m.b = __ddiv_rn(__dadd_rn((double)cnt[2], (double)cnt[1]), tot);         // (:136-137)
            m.oa = __dsub_rn(1.0, m.a);
            m.ob = __dsub_rn(1.0, m.b);
            atomicAdd(&n_used[snp % TESTED_SHARDS], 1ull);
        }
        miss = m;
        params[snp] = m;
    }
    __syncthreads();
    const SnpVals m = miss;
    SnpVals* out = vals + (uint64_t)snp * Sv;
    for (uint32_t s = threadIdx.x; s < Sv; s += blockDim.x) {
        if (s >= S) {
            out[s] = SnpVals{0.0, 0.0, 0.0, 0.0};
            continue;
        }
        const uint32_t d = (row[s >> 2] >> (2u * (s & 3u))) & 3u;
        SnpVals v;
        if (d == 1u)
            v = m;
        else {
            v.a = d == 3u ? 1.0 : 0.0;
            v.b = d >= 2u ? 1.0 : 0.0;
            v.oa = d == 3u ? 0.0 : 1.0;
            v.ob = d >= 2u ? 0.0 : 1.0;
        }
        out[s] = v;
    }
}

// tiles[blockIdx.x] = (first row, first column) of a tile that holds at least one pair r > c. sums[r * S + c], r > c.
template <int RW>
__global__ void __launch_bounds__(64) snpkin_accumulate_kernel(const uint8_t* __restrict__ bed, uint32_t bytes_per_snp, uint32_t n_snps,
                                                               uint32_t S, uint32_t Sv, const SnpVals* __restrict__ params,
                                                               const SnpVals* __restrict__ vals, const uint2* __restrict__ tiles,
                                                               double* __restrict__ sums) {
    const uint2 t = tiles[blockIdx.x];
    const uint32_t c = t.y + threadIdx.x;
    const uint32_t cc = c < S ? c : S - 1;  // lanes past the last sample decode a real one and store nothing
    const uint32_t cbyte = cc >> 2, cshift = 2u * (cc & 3u);
    double acc[RW];
#pragma unroll
    for (int k = 0; k < RW; k++) {
        const uint32_t r = t.x + k;
        acc[k] = (r < S && c < r) ? sums[(uint64_t)r * S + c] : 0.0;
    }
    // The lane's .bed bytes are loaded a group of U SNPs ahead (a load's latency is far longer than a SNP's arithmetic).
    constexpr int U = 8;
    uint32_t next[U];
#pragma unroll
    for (int u = 0; u < U; u++) next[u] = bed[(uint64_t)min((uint32_t)u, n_snps - 1) * bytes_per_snp + cbyte];
    for (uint32_t i0 = 0; i0 < n_snps; i0 += U) {
        uint32_t cur[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            cur[u] = next[u];
            next[u] = bed[(uint64_t)min(i0 + U + u, n_snps - 1) * bytes_per_snp + cbyte];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = i0 + u;
            if (i >= n_snps) break;
            const SnpVals p = params[i];
            const uint32_t d = (cur[u] >> cshift) & 3u;
            const bool miss = d == 1u, alt = d == 3u, called = d >= 2u;  // the column's values, as in prep
            const double ca = miss ? p.a : (alt ? 1.0 : 0.0), coa = miss ? p.oa : (alt ? 0.0 : 1.0);
            const double cb = miss ? p.b : (called ? 1.0 : 0.0), cob = miss ? p.ob : (called ? 0.0 : 1.0);
            const SnpVals* vi = vals + (uint64_t)i * Sv + t.x;
#pragma unroll
            for (int k = 0; k < RW; k++) {
                const SnpVals r = vi[k];
                acc[k] = __dadd_rn(acc[k], __dadd_rn(__dmul_rn(r.a, ca), __dmul_rn(r.oa, coa)));  // pass A (:49-50)
                acc[k] = __dadd_rn(acc[k], __dadd_rn(__dmul_rn(r.b, cb), __dmul_rn(r.ob, cob)));  // pass B
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RW; k++) {
        const uint32_t r = t.x + k;
        if (r < S && c < r) sums[(uint64_t)r * S + c] = acc[k];
    }
}

}  // namespace

uint32_t snpkin_vals_stride(uint32_t S) { return S + 8; }
size_t snpkin_vals_bytes(uint32_t S, uint32_t chunk_snps) { return (size_t)chunk_snps * snpkin_vals_stride(S) * sizeof(SnpVals); }
size_t snpkin_params_bytes(uint32_t chunk_snps) { return (size_t)chunk_snps * sizeof(SnpVals); }

hipError_t launch_snpkin_prep(const uint8_t* bed, uint32_t n_snps, uint32_t bytes_per_snp, uint32_t S, void* params, void* vals,
                              unsigned long long* n_used, hipStream_t st) {
    if (n_snps == 0) return hipSuccess;
    hipLaunchKernelGGL(snpkin_prep_kernel, dim3(n_snps), dim3(256), 0, st, bed, bytes_per_snp, S, snpkin_vals_stride(S), static_cast<SnpVals*>(params),
                       static_cast<SnpVals*>(vals), n_used);
    return hipGetLastError();
}

hipError_t launch_snpkin_accumulate(int rows_per_wave, const uint8_t* bed, uint32_t n_snps, uint32_t bytes_per_snp, uint32_t S,
                                    const void* params, const void* vals, const uint2* tiles, uint32_t n_tiles, double* sums,
                                    hipStream_t st) {
    if (n_snps == 0 || n_tiles == 0) return hipSuccess;
    const SnpVals* p = static_cast<const SnpVals*>(params);
    const SnpVals* v = static_cast<const SnpVals*>(vals);
    if (rows_per_wave == 8)
        hipLaunchKernelGGL(snpkin_accumulate_kernel<8>, dim3(n_tiles), dim3(64), 0, st, bed, bytes_per_snp, n_snps, S, snpkin_vals_stride(S), p, v, tiles, sums);
    else
        hipLaunchKernelGGL(snpkin_accumulate_kernel<4>, dim3(n_tiles), dim3(64), 0, st, bed, bytes_per_snp, n_snps, S, snpkin_vals_stride(S), p, v, tiles, sums);
    return hipGetLastError();
}

}  // namespace kgwas
