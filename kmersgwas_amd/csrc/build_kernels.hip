// build_kernels.hip — device side of build_kmers_table (src/kmers_merge_multiple_databaes.cpp:88-121): the presence/absence
// rows of one piece of the all-k-mers list.
//
// A piece is a run of whole key windows of the reference whose all-k-mers words A[0, n) do not descend (build_table.cpp sends
// every other piece to the host). The reference's hash map of a window keeps the first insert of a key; in a non-descending A
// that is lower_bound(A, x), so an accession's word x sets its bit in row lower_bound(A, x) iff that row's key equals x
// (DESIGN.md §4.9). bt_init writes the rows' keys and zeroes their bits; bt_match takes one block of one accession's words,
// one lane per word, and ORs the accession's bit into the rows it finds.
#include <algorithm>

#include "kernels.h"
#include "sorted_search.h"

namespace kgwas {

namespace {

constexpr uint32_t BT_BLOCK = 256;
constexpr uint64_t BT_KEY_MASK = 0x3FFFFFFFFFFFFFFFull;  // the top two bits of a word are strand flags (src/kmers_single_database.cpp:147)

// A[r] &= mask; rows[r] = [A[r]][stride - 1 zero words]. One lane per output word.
__global__ void __launch_bounds__(BT_BLOCK) bt_init_kernel(uint64_t* A, uint64_t n, uint64_t stride, uint64_t* rows) {
    const uint64_t i = (uint64_t)blockIdx.x * BT_BLOCK + threadIdx.x;
    if (i >= n * stride) return;
    const uint64_t r = i / stride, w = i - r * stride;
    uint64_t v = 0;
    if (w == 0) {
        v = A[r] & BT_KEY_MASK;
        A[r] = v;
    }
    rows[i] = v;
}

// Words slice[0, m) of one accession (raw: the flags are masked here) against the piece's keys A[0, n) (masked, non-descending;
// spl[j] = A[j * B] staged in LDS): where A[lower_bound(A, x)] == x the accession's bit is ORed into that row's word - a 64-bit
// vector atomic, because lanes of other launches (other accessions of the same 64) write the same words. *descends is set
// when a word is below the one before it (carry_key before word 0 when has_prev: the last word of the slice's previous block).
__global__ void __launch_bounds__(BT_BLOCK) bt_match_kernel(const uint64_t* A, uint64_t n, const uint64_t* spl_g, uint32_t ns, uint64_t B,
                                                            const uint64_t* slice, uint32_t m, uint64_t carry_key, int has_prev,
                                                            uint64_t* rows, uint64_t stride, uint32_t word, unsigned long long bit,
                                                            uint32_t* descends) {
    __shared__ uint64_t spl[FK_SPLITTERS];
    for (uint32_t i = threadIdx.x; i < ns; i += BT_BLOCK) spl[i] = spl_g[i];
    __syncthreads();
    for (uint32_t j = blockIdx.x * BT_BLOCK + threadIdx.x; j < m; j += gridDim.x * BT_BLOCK) {
        const uint64_t x = slice[j] & BT_KEY_MASK;
        if (j > 0 || has_prev) {
            const uint64_t px = j > 0 ? (slice[j - 1] & BT_KEY_MASK) : carry_key;
            if (x < px) *descends = 1u;
        }
        const uint64_t lb = fk_list_bound<false>(spl, ns, A, n, B, x);
        if (lb < n && A[lb] == x) atomicOr(reinterpret_cast<unsigned long long*>(rows + lb * stride + 1 + word), bit);
    }
}

}  // namespace

hipError_t launch_bt_init(uint64_t* A, uint64_t n, uint64_t stride, uint64_t* rows, hipStream_t st) {
    const uint64_t total = n * stride;
    if (total == 0) return hipSuccess;
    const uint64_t blocks = (total + BT_BLOCK - 1) / BT_BLOCK;
    if (stride < 2 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bt_init_kernel, dim3((uint32_t)blocks), dim3(BT_BLOCK), 0, st, A, n, stride, rows);
    return hipGetLastError();
}

hipError_t launch_bt_match(const uint64_t* A, uint64_t n, const uint64_t* spl, uint32_t ns, uint64_t B, const uint64_t* slice,
                           uint32_t m, uint64_t carry_key, bool has_prev, uint64_t* rows, uint64_t stride, uint64_t accession,
                           uint32_t* descends, hipStream_t st) {
    if (m == 0 || n == 0) return hipSuccess;
    // the splitters must cover A: spl[j] = A[j * B] for every j with j * B < n
    if (ns == 0 || ns > FK_SPLITTERS || B == 0 || (uint64_t)ns != (n + B - 1) / B || accession / 64 + 1 >= stride) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)m + BT_BLOCK - 1) / BT_BLOCK, 2048));
    hipLaunchKernelGGL(bt_match_kernel, dim3(grid), dim3(BT_BLOCK), 0, st, A, n, spl, ns, B, slice, m, carry_key, has_prev ? 1 : 0, rows,
                       stride, (uint32_t)(accession / 64), 1ull << (accession % 64), descends);
    return hipGetLastError();
}

}  // namespace kgwas
