// sorted_search.h — device-side binary searches in a sorted list of 64-bit keys, shared by filter_kernels.hip (table rows
// searched in the k-mer list) and build_kernels.hip (an accession's k-mers searched in the all-k-mers piece).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kgwas {

// First index in [lo, hi) with a[i] >= x (lower) or a[i] > x (upper); hi when there is none.
template <bool UPPER, class P>
__device__ __forceinline__ uint64_t fk_bound(P a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = a[mid];
        if (UPPER ? (v <= x) : (v < x))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// bound over the whole list: the splitters spl[j] = L[j * B] (j < ns) in LDS narrow it to one block of B - 1 entries in HBM
template <bool UPPER>
__device__ __forceinline__ uint64_t fk_list_bound(const uint64_t* spl, uint32_t ns, const uint64_t* L, uint64_t n, uint64_t B,
                                                  uint64_t x) {
    const uint64_t j = fk_bound<UPPER>(spl, 0, ns, x);  // splitters on the "before" side of x
    if (j == 0) return 0;
    const uint64_t lo = (j - 1) * B + 1, hi = j * B < n ? j * B : n;
    return fk_bound<UPPER>(L, lo, hi, x);
}

}  // namespace kgwas
