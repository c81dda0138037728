// Launch arguments of the TRAIN head's own kernels (train_head.hip, wgrad.hip) and the column-sum core they share with
// train_backbone.hip; the C ABI is in include/ssd_hip.h.
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

static inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
static inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

// a 256-thread launch inside an entry point (host.h's HIPCHK returns on an error)
#define LAUNCH(kernel, grid, s, ...)                                  \
    do {                                                              \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, __VA_ARGS__); \
        HIPCHK(hipGetLastError());                                    \
    } while (0)

// ----------------------------------------------------------------------------- the column-sum core
// Sums over the rows of a [rows][C] tensor, per column, in double and in an order fixed by the shapes alone (include/ssd_hip.h:
// the batch norm's slab order): the batch norm's statistics and dbias (train_head.hip), the depthwise and the first convolution's
// weight gradients (train_backbone.hip).  The rows are cut into slabs of `slab_rows`; block = slab.  Thread (rl = tid / G,
// g = tid % G) of a block's 256 walks the rows r0 + rl, r0 + rl + rpp, ... of its slab for the channel quad g (G quads, rpp = 256 / G
// rows per pass), adding in double; the block then adds its rpp row lanes in ascending order (slab_reduce4) and writes one double per
// column and slab; the second stage (launch_slab_sum, or stat_final where it does more than sum) adds the slabs in ascending order.
#define TH_STAT_COLS 1024  // channels one block covers (256 threads x 4)

// The slab rule for a tensor of R rows of G channel quads (1 <= G <= 256): about 1024 blocks in all, a slab a whole number of passes
// and at least 8 of them: slab_rows = max(8 * rpp, ceil(R / 1024)) rounded up to a multiple of rpp.  The result is what the
// tensor's kernels take; a level list (train_head.hip make_slabs) applies the rule to the rows of all its levels together.
struct Slabs {
    long long R;
    int slab_rows, n_slabs;
};
static inline Slabs slab_rule(long long R, int G)
{
    const int rpp = 256 / G;
    long long sr = (R + 1023) / 1024;
    if (sr < 8LL * rpp) sr = 8LL * rpp;
    sr = (sr + rpp - 1) / rpp * rpp;
    return {R, (int)sr, (int)((R + sr - 1) / sr)};
}

// out[i] = fp32(partial[i] + partial[stride + i] + ... + partial[(n_slabs - 1) * stride + i]), i < n: added in double in ascending
// slab order, rounded once (train_head.hip)
hipError_t launch_slab_sum(const double *partial, int n_slabs, long long stride, int n, float *out, hipStream_t s);

#ifdef __HIPCC__
typedef float v4f __attribute__((ext_vector_type(4)));

typedef float v2f __attribute__((ext_vector_type(2)));

// 4 consecutive channels of a row from channel c on (c % 4 == 0), by the widest access the row width allows (th_width): one 16-byte
// access where C % 4 == 0 (the quad is inside or outside as a whole), two 8-byte accesses where C % 4 == 2 (every row start and
// every channel pair is 8-byte aligned; the second pair of the last quad is outside), else element by element; channels beyond C
// read 0 / are not written
static __device__ inline int th_width(int C) { return (C & 3) == 0 ? 4 : (C & 1) == 0 ? 2 : 1; }
static __device__ inline v4f th_load4(const float *row, int c, int C, int vec)
{
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (vec == 4) {
        if (c < C) v = *(const v4f *)(row + c);
    } else if (vec == 2) {
        if (c < C) { const v2f t = *(const v2f *)(row + c); v[0] = t[0]; v[1] = t[1]; }
        if (c + 2 < C) { const v2f t = *(const v2f *)(row + c + 2); v[2] = t[0]; v[3] = t[1]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) v[e] = row[c + e];
    }
    return v;
}
static __device__ inline void th_store4(float *row, int c, int C, int vec, v4f v)
{
    if (vec == 4) {
        if (c < C) *(v4f *)(row + c) = v;
    } else if (vec == 2) {
        if (c < C) *(v2f *)(row + c) = (v2f){v[0], v[1]};
        if (c + 2 < C) *(v2f *)(row + c + 2) = (v2f){v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) row[c + e] = v[e];
    }
}

// a thread's place in its block's slab (slab: counted within its tensor): the row lane rl, the first channel c of its quad
// g = tid % G within the block's columns, the rows [r0, r1) of the slab, and whether the lane walks rows at all (256 % G lanes of
// a block idle)
struct SlabLane {
    int rl, c, rpp;
    long long r0, r1;
    bool on;
};
static __device__ inline SlabLane slab_lane(int tid, int G, int slab, int slab_rows, long long rows)
{
    SlabLane t;
    t.rpp = 256 / G;
    t.rl = tid / G;
    t.c = (tid - t.rl * G) << 2;
    t.r0 = (long long)slab * slab_rows;
    t.r1 = t.r0 + slab_rows < rows ? t.r0 + slab_rows : rows;
    t.on = t.rl < t.rpp;
    return t;
}

// The in-block reduction of one quantity: every thread of the block hands in its quad's four sums (idle lanes: zeros, never read),
// sm holds 1024 doubles.  Column i of the block's 4 * G is then the sum over j of lane (j, i / 4)'s element i % 4, j = 0 .. rpp - 1
// ASCENDING from +0, by thread i, i + 256, ...: sm is read and dst written at consecutive addresses, for any rpp >= 1.  Column
// c0 + i of the tensor goes to dst[c0 + i] where it is below C (the batch norm takes C % 4 != 0).  There is no barrier behind the
// reads: a caller that hands in the same sm again puts a __syncthreads() between the two calls.
static __device__ inline void slab_reduce4(double *sm, const double (&acc)[4], int tid, int G, double *dst, int c0, int C)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[tid * 4 + e] = acc[e];
    __syncthreads();
    const int n = G << 2, rpp = 256 / G;
    for (int i = tid; i < n; i += 256) {
        double s = 0.0;
        for (int j = 0; j < rpp; ++j) s += sm[j * n + i];
        if (c0 + i < C) dst[c0 + i] = s;
    }
}
#endif

// The bodies of the convolution, batch-norm (train_head.hip) and depthwise (train_backbone.hip) entry points; `fn` names the entry
// point in ssd_last_error().  The last flag of each is set by the TRAIN ShuffleNet's entry points (train_shufflenet.hip) alone and
// lifts one refusal: even_cin -- k = 1 takes any even Cin; pw_dx -- k = 1 gives the data gradient; none_ok -- the batch norm takes
// SSD_ACT_NONE; even_c -- the depthwise calls take any even C.  Without the flag: the arguments, refusals and bits of before.
#include <string>
size_t conv_train_workspace(const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride, bool pw_dx, bool even_cin);
int conv_train_forward(const std::string &fn, const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride,
                       const float *w_dev, const float *bias_dev, const float *const *up_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream, bool even_cin = false);
int conv_train_backward(const std::string &fn, const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride,
                        const float *w_dev, float *dw_dev, float *dbias_dev, void *workspace_dev, size_t workspace_bytes, void *stream,
                        bool pw_dx = false, bool even_cin = false);
int bn_train_forward(const std::string &fn, const ssd_bn_level *levels, int n_levels, int C, int act, int training, float epsilon,
                     float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream, bool none_ok = false);
int bn_train_backward(const std::string &fn, const ssd_bn_level *levels, int n_levels, int C, int act, void *workspace_dev,
                      size_t workspace_bytes, void *stream, bool none_ok = false);
int dw_train_forward(const std::string &fn, const float *x_dev, int B, int H, int W, int C, const float *w_dev, int stride, float *out_dev,
                     void *stream, bool even_c);
size_t dw_train_workspace(int B, int H, int W, int C, int stride, bool even_c);
int dw_train_backward(const std::string &fn, const float *x_dev, const float *dy_dev, int B, int H, int W, int C, const float *w_dev, int stride,
                      float *dx_dev, float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream, bool even_c);

// train_head.hip: the column statistics of a level list and the batch norm.  A slab never crosses a level.
struct StatLevel {
    ssd_bn_level p;        // the caller's level (dbias: x = a level's dy)
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
    int act;               // SSD_ACT_RELU | SSD_ACT_RELU6: the gate of the batch norm's activation; SSD_ACT_NONE (the TRAIN ShuffleNet): none
};
