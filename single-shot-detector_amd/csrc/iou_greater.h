// The NMS rule's one comparison, shared by the detector's per-class NMS (postprocess.hip K9c) and the merge of tiled detection
// (tiles.hip): device only, every operation separately rounded (-ffp-contract=off).
#pragma once
#include "ssd_internal.h"

typedef float v4f __attribute__((ext_vector_type(4)));

// IOUGreaterThanThreshold of TF r1.12 non_max_suppression_op.cc
__device__ __forceinline__ bool iou_greater(const v4f bi, const v4f bj, float thr)
{
    const float ymin_i = fminf(bi[0], bi[2]), xmin_i = fminf(bi[1], bi[3]);
    const float ymax_i = fmaxf(bi[0], bi[2]), xmax_i = fmaxf(bi[1], bi[3]);
    const float ymin_j = fminf(bj[0], bj[2]), xmin_j = fminf(bj[1], bj[3]);
    const float ymax_j = fmaxf(bj[0], bj[2]), xmax_j = fmaxf(bj[1], bj[3]);
    const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
    const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
    // branch-free form of `if (area_i <= 0 || area_j <= 0) return false;` -- with both areas
    // positive the union is positive, otherwise the (possibly NaN) quotient is masked.
    const bool valid = (area_i > 0.0f) & (area_j > 0.0f);
    const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
    const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
    const float ih = fmaxf(iy1 - iy0, 0.0f), iw = fmaxf(ix1 - ix0, 0.0f);
    const float inter = ih * iw;
    float uni = area_i + area_j;
    uni = uni - inter;
    const float iou = inter / uni;
    return valid & (iou > thr);
}
