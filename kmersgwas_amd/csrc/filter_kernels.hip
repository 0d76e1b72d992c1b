// filter_kernels.hip — device side of filter_kmers (src/filter_kmers.cpp:152-177): match a piece of table rows against the
// sorted k-mer list, compact the rows the reference's merge-join emits, and turn them into its text lines.
//
// The merge-join over a non-decreasing run of keys is parallel: row r is emitted iff rank-in-run(r) < count(L, x_r), where
// rank-in-run is the number of earlier rows with the same key. fk_match_kernel gives every row its
// count and a run-head mark, a max-scan turns the marks into each row's run start, fk_flag_kernel applies the rule up to
// the piece's first descent (the host carries on from there), and a DeviceSelect compacts the emitted offsets.
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "sorted_search.h"

namespace kgwas {

namespace {

constexpr uint32_t FK_BLOCK = 256;

// Per row: lb = lower_bound(L, x), cnt = count(L, x), head = r + 1 where the key differs from the previous row's (0 else),
// and the first descent (key < previous key) of the piece into *first_desc (atomicMin; 0xFFFFFFFF = none).
// Row 0's previous key is the carry (the last key of the previous piece) when has_prev.
__global__ void __launch_bounds__(FK_BLOCK) fk_match_kernel(const uint64_t* rows, uint64_t stride, uint32_t n_rows,
                                                            const uint64_t* L, uint64_t n, const uint64_t* spl_g, uint32_t ns,
                                                            uint64_t B, uint64_t carry_key, int has_prev, uint64_t* lb_out,
                                                            uint64_t* cnt_out, uint32_t* head_out, uint32_t* first_desc) {
    __shared__ uint64_t spl[FK_SPLITTERS];
    for (uint32_t i = threadIdx.x; i < ns; i += FK_BLOCK) spl[i] = spl_g[i];
    __syncthreads();
    for (uint32_t r = blockIdx.x * FK_BLOCK + threadIdx.x; r < n_rows; r += gridDim.x * FK_BLOCK) {
        const uint64_t x = rows[(uint64_t)r * stride];
        const bool prev = r > 0 || has_prev;
        const uint64_t px = r > 0 ? rows[(uint64_t)(r - 1) * stride] : carry_key;
        const uint64_t lb = fk_list_bound<false>(spl, ns, L, n, B, x);
        const uint64_t ub = fk_list_bound<true>(spl, ns, L, n, B, x);
        lb_out[r] = lb;
        cnt_out[r] = ub - lb;
        head_out[r] = (!prev || x != px) ? r + 1 : 0u;
        if (prev && x < px) atomicMin(first_desc, r);
    }
}

// emit[r] = r < first descent && rank-in-run(r) < count(L, x_r). run_start[r] = max-scan of head (0: the run began in an
// earlier piece, carry_run rows ago). Writes info: [0] run length of the piece's last row, [1] the last key, and, when the
// piece descends at row d > 0, [2] the run length of row d - 1 and [3] its key.
__global__ void __launch_bounds__(FK_BLOCK) fk_flag_kernel(const uint64_t* rows, uint64_t stride, uint32_t n_rows,
                                                           const uint64_t* cnt, const uint32_t* run_start, uint64_t carry_run,
                                                           const uint32_t* first_desc, uint8_t* emit, uint64_t* info) {
    const uint32_t d = *first_desc;
    for (uint32_t r = blockIdx.x * FK_BLOCK + threadIdx.x; r < n_rows; r += gridDim.x * FK_BLOCK) {
        const uint32_t s = run_start[r];
        const uint64_t rank = s ? (uint64_t)(r - (s - 1)) : carry_run + r;
        emit[r] = (r < d && rank < cnt[r]) ? 1 : 0;
        if (r == n_rows - 1) {
            info[0] = rank + 1;
            info[1] = rows[(uint64_t)r * stride];
        }
        if (d < n_rows && r + 1 == d) {
            info[2] = rank + 1;
            info[3] = rows[(uint64_t)r * stride];
        }
    }
}

// keys[i] = the key of row r0 + i (the host's merge-join after a descent)
__global__ void __launch_bounds__(FK_BLOCK) fk_keys_kernel(const uint64_t* rows, uint64_t stride, uint32_t r0, uint32_t n_rows,
                                                           uint64_t* keys) {
    const uint32_t i = blockIdx.x * FK_BLOCK + threadIdx.x;
    if (r0 + i < n_rows && i < n_rows) keys[i] = rows[(uint64_t)(r0 + i) * stride];
}

// out[i] = row sel[i] of the piece, all 1 + W_f words (one lane per word)
__global__ void __launch_bounds__(FK_BLOCK) fk_gather_kernel(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m,
                                                             uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * FK_BLOCK + threadIdx.x;
    if (i >= (uint64_t)m * stride) return;
    const uint64_t line = i / stride, w = i - line * stride;
    out[i] = rows[(uint64_t)sel[line] * stride + w];
}

// The text of lines [0, m): line i = bits2kmer31(key, k) (src/kmer_general.cpp:77-87), "\t0" / "\t1" per accession in
// file column order, "\n" - width k + 2 S_f + 1 bytes, at i * width. Each lane builds 16 consecutive bytes and writes
// them with one 16-byte store; the buffer is allocated to a multiple of 16 (the bytes past m * width are not used).
__global__ void __launch_bounds__(FK_BLOCK) fk_format_kernel(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m,
                                                             uint32_t k, uint32_t S_f, uint64_t width, uint4* out) {
    const uint64_t lane = (uint64_t)blockIdx.x * FK_BLOCK + threadIdx.x;
    const uint64_t total = (uint64_t)m * width;
    const uint64_t o = lane * 16;
    if (o >= total) return;
    uint64_t line = o / width, j = o - line * width;
    const uint64_t* row = rows + (uint64_t)sel[line] * stride;
    uint32_t dw[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) {
        uint32_t c = 0;
        if (o + b < total) {
            if (j < k)
                c = (uint32_t)"ACGT"[(row[0] >> (2 * (k - 1 - j))) & 3];
            else if (j < (uint64_t)k + 2ull * S_f) {
                const uint64_t t = j - k;
                if (t & 1) {
                    const uint64_t col = t >> 1;
                    c = '0' + (uint32_t)((row[1 + (col >> 6)] >> (col & 63)) & 1);
                } else
                    c = '\t';
            } else
                c = '\n';
            if (++j == width && o + b + 1 < total) {
                j = 0;
                line++;
                row = rows + (uint64_t)sel[line] * stride;
            }
        }
        dw[b >> 2] |= c << (8 * (b & 3));
    }
    out[lane] = make_uint4(dw[0], dw[1], dw[2], dw[3]);
}

uint32_t fk_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + FK_BLOCK - 1) / FK_BLOCK, 2048)); }

}  // namespace

hipError_t launch_fk_match(const uint64_t* rows, uint64_t stride, uint32_t n_rows, const uint64_t* L, uint64_t n,
                           const uint64_t* spl, uint32_t ns, uint64_t B, uint64_t carry_key, bool has_prev, uint64_t* lb,
                           uint64_t* cnt, uint32_t* head, uint32_t* first_desc, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    if (ns == 0 || ns > FK_SPLITTERS || n == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fk_match_kernel, dim3(fk_grid(n_rows)), dim3(FK_BLOCK), 0, st, rows, stride, n_rows, L, n, spl, ns, B,
                       carry_key, has_prev ? 1 : 0, lb, cnt, head, first_desc);
    return hipGetLastError();
}

size_t fk_scan_temp_bytes(uint32_t max_rows) {
    size_t a = 0, b = 0;
    if (hipcub::DeviceScan::InclusiveScan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), max_rows) !=
            hipSuccess ||
        hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<uint32_t>(0), (const uint8_t*)nullptr, (uint32_t*)nullptr,
                                      (uint32_t*)nullptr, max_rows) != hipSuccess)
        return 0;
    return std::max(a, b);
}

hipError_t launch_fk_select(const uint64_t* rows, uint64_t stride, uint32_t n_rows, const uint64_t* cnt, const uint32_t* head,
                            uint32_t* run_start, uint64_t carry_run, const uint32_t* first_desc, uint8_t* emit, uint32_t* sel,
                            uint32_t* n_sel, uint64_t* info, void* temp, size_t temp_bytes, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    hipError_t e;
    size_t tb = temp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveScan(temp, tb, head, run_start, hipcub::Max(), n_rows, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(fk_flag_kernel, dim3(fk_grid(n_rows)), dim3(FK_BLOCK), 0, st, rows, stride, n_rows, cnt, run_start, carry_run,
                       first_desc, emit, info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = temp_bytes;
    return hipcub::DeviceSelect::Flagged(temp, tb, hipcub::CountingInputIterator<uint32_t>(0), emit, sel, n_sel, n_rows, st);
}

hipError_t launch_fk_keys(const uint64_t* rows, uint64_t stride, uint32_t r0, uint32_t n_rows, uint64_t* keys, hipStream_t st) {
    if (r0 >= n_rows) return hipSuccess;
    hipLaunchKernelGGL(fk_keys_kernel, dim3((n_rows - r0 + FK_BLOCK - 1) / FK_BLOCK), dim3(FK_BLOCK), 0, st, rows, stride, r0, n_rows,
                       keys);
    return hipGetLastError();
}

hipError_t launch_fk_gather(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m, uint64_t* out, hipStream_t st) {
    const uint64_t n = (uint64_t)m * stride;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fk_gather_kernel, dim3((uint32_t)((n + FK_BLOCK - 1) / FK_BLOCK)), dim3(FK_BLOCK), 0, st, rows, stride, sel, m,
                       out);
    return hipGetLastError();
}

hipError_t launch_fk_format(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m, uint32_t k, uint32_t S_f,
                            void* text, hipStream_t st) {
    const uint64_t width = (uint64_t)k + 2ull * S_f + 1, lanes = ((uint64_t)m * width + 15) / 16;
    if (lanes == 0) return hipSuccess;
    if ((lanes + FK_BLOCK - 1) / FK_BLOCK > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fk_format_kernel, dim3((uint32_t)((lanes + FK_BLOCK - 1) / FK_BLOCK)), dim3(FK_BLOCK), 0, st, rows, stride, sel,
                       m, k, S_f, width, reinterpret_cast<uint4*>(text));
    return hipGetLastError();
}

}  // namespace kgwas
