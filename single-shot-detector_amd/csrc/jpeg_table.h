// The search both JPEG device stages (jpeg.hip, jpeg_enc.hip) make in their batch tables: which image holds block or tile g.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the last row i of a table with begin(i) <= g, begin ascending from 0, g below the batch's total
template <class Begin>
__device__ __forceinline__ int find_row(int B, int64_t g, Begin begin)
{
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (begin(mid) <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
