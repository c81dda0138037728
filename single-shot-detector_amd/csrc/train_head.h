// Launch arguments of the TRAIN head's own kernels (train_head.hip, wgrad.hip); the C ABI is in include/ssd_hip.h.
#pragma once
#include "../../include/ssd_hip.h"
#include "ssd_internal.h"

#define TH_MAX_LEVELS 8

// wgrad.hip
struct WgradLevel {
    const float *x, *dy;   // logical NHWC [B,H,W,Cin], [B,OH,OW,Cout]
    int H, W;              // the input's size
    int OW, P, R;          // output width, P = OH*OW positions per image, R = B*P rows: K runs over OUTPUT positions
    int slice_begin;       // first K-slice of this level
    UDiv dP, dOW;
};
struct WgradArgs {
    WgradLevel lv[TH_MAX_LEVELS];
    int nlevels, Cin, Cout;
    int k, stride, pad;    // tap (kh,kw) of output (oy,ox) reads x[oy*stride + kh - pad, ox*stride + kw - pad], zero outside
    int rows_per_slice, n_slices, tiles_ci;
    float *partial;        // [n_slices][k*k][Cin][Cout]
};
int wgrad_tile_n(int Cout);
hipError_t launch_wgrad(const WgradArgs &a, float *dw, hipStream_t s);

// 4 consecutive channels of a row from channel c on: one 16-byte access where C % 4 == 0 (c % 4 == 0, so the quad is inside or
// outside as a whole), else element by element; channels beyond C read 0 / are not written
#ifdef __HIPCC__
typedef float th_v4f __attribute__((ext_vector_type(4)));
static __device__ inline th_v4f th_load4(const float *row, int c, int C, bool vec)
{
    th_v4f v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (c < C) v = *(const th_v4f *)(row + c);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) v[e] = row[c + e];
    }
    return v;
}
static __device__ inline void th_store4(float *row, int c, int C, bool vec, th_v4f v)
{
    if (vec) {
        if (c < C) *(th_v4f *)(row + c) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) row[c + e] = v[e];
    }
}
#endif

#define TH_STAT_COLS 1024  // channels one block of the column statistics covers (256 threads x 4)
// train_head.hip: column statistics and the batch norm.  A level's rows are cut into slabs of `slab_rows`; block = slab.
struct StatLevel {
    ssd_bn_level p;        // the caller's level (dbias: x = a level's dy, lv[0].out = dbias)
    int slab_begin, n_slabs;
    float unbias;          // (float)(rows / (rows - 1)), 1 when rows == 1
};
struct StatArgs {
    StatLevel lv[TH_MAX_LEVELS];
    int nlevels, C, slab_rows, n_slabs;
    int CW;                // columns a block covers: min(C, TH_STAT_COLS); blockIdx.y of stat_partial picks the chunk (dbias of wide layers)
    double *partial;       // [n_slabs][2][C]
    float eps, one_minus_momentum;
    int training;
    int act;               // SSD_ACT_RELU | SSD_ACT_RELU6: the gate of the batch norm's activation
};
