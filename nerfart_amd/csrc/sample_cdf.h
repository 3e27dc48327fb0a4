// sample_cdf.h - the searches and the piece-wise linear inverse CDF of the per-ray samplers, and the test that lets k_upsample leave out its sort.
// No HIP in here: tests/test_upsample_sorted_host.py compiles this header as host code.
#pragma once
#include <string.h>

#if defined(__HIPCC__)
#define NERFART_HD __device__ __forceinline__
#else
#define NERFART_HD inline
#endif

namespace nerfart {

// first index i in [0, n] with c[i] >= u  (torch.searchsorted(..., right=False))
NERFART_HD int lower_bound(const float* c, int n, float u) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] < u) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index i in [0, n] with c[i] > u
NERFART_HD int upper_bound(const float* c, int n, float u) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Piece-wise linear inverse CDF of one sample (utils/rend_util.py:276-291): bracket by lower
// bound, clamp to the array, a denominator below 1e-5 becomes 1.
NERFART_HD float invert_cdf_at(const float* bins, const float* cdf, int n, float u) {
    const int idx = lower_bound(cdf, n, u);
    const int below = idx - 1 < 0 ? 0 : idx - 1;
    const int above = idx > n - 1 ? n - 1 : idx;
    const float c0 = cdf[below], c1 = cdf[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.f;
    const float t = (u - c0) / denom;
    const float b0 = bins[below], b1 = bins[above];
    return b0 + t * (b1 - b0);
}

// Lane `lane` of 64 looks at its elements j = lane, lane + 64, ... of a row: is every one of them in place against its right neighbour?  "In place" is
// a[j] < a[j + 1], or the two are the same number in the same bits.  False for a NaN on either side, and for +0 next to -0: a row that passes on all
// 64 lanes is ascending, NaN-free, and its equal elements are indistinguishable, so a comparison sort of it - bitonic_sort included, whose descending
// stages exchange equal elements - returns the same bits.
NERFART_HD bool lane_row_in_order(const float* a, int n, int lane) {
    bool ok = true;
    for (int j = lane; j + 1 < n; j += 64) {
        const float x = a[j], y = a[j + 1];
        unsigned xb, yb;
        memcpy(&xb, &x, 4); memcpy(&yb, &y, 4);
        ok = ok && (x < y || (x == y && xb == yb));
    }
    return ok;
}

}  // namespace nerfart
