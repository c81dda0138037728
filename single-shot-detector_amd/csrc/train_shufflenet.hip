// The TRAIN ShuffleNet (include/ssd_hip.h, the block of that name): what ShuffleNet-v2 in TRAIN mode needs beyond the TRAIN backbone's
// calls.  The depthwise, pointwise and batch-norm entry points here are the TRAIN backbone's bodies (train_head.h) with the one flag
// that lifts a refusal -- any even channel count on 8-byte accesses, SSD_ACT_NONE -- so that the old entry points keep theirs.  The
// kernels of this file are the copies of the graph (concat_shuffle_split and its transpose, the closing concat and its split: index
// arithmetic, no table, no upload) and the gradient of the 3x3 stride-2 max pool (a gather, no atomics).
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`.
#include "host.h"
#include "train_head.h"

#include <algorithm>

// ----------------------------------------------------------------------------- depthwise, pointwise, batch norm: the flagged bodies
extern "C" int ssd_sn_depthwise_train_forward(const float *x_dev, int32_t B, int32_t H, int32_t W, int32_t C, const float *w_dev,
                                              int32_t stride, float *out_dev, void *stream)
{
    return dw_train_forward("ssd_sn_depthwise_train_forward", x_dev, B, H, W, C, w_dev, stride, out_dev, stream, true);
}

extern "C" size_t ssd_sn_depthwise_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride)
{
    return dw_train_workspace(B, H, W, C, stride, true);
}

extern "C" int ssd_sn_depthwise_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                                               const float *w_dev, int32_t stride, float *dx_dev, float *dw_dev, void *workspace_dev,
                                               size_t workspace_bytes, void *stream)
{
    return dw_train_backward("ssd_sn_depthwise_train_backward", x_dev, dy_dev, B, H, W, C, w_dev, stride, dx_dev, dw_dev, workspace_dev,
                             workspace_bytes, stream, true);
}

static const char *sn_pw_sizes(int Cin, int Cout) { return (Cin < 2 || Cout < 2 || (Cin | Cout) & 1) ? "Cin and Cout must be even" : nullptr; }

extern "C" size_t ssd_sn_pointwise_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout)
{
    return sn_pw_sizes(Cin, Cout) ? 0 : conv_train_workspace(levels, n_levels, B, Cin, Cout, 1, 1, true, true);
}

extern "C" int ssd_sn_pointwise_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                              const float *w_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (const char *why = sn_pw_sizes(Cin, Cout)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_sn_pointwise_train_forward: ") + why);
    return conv_train_forward("ssd_sn_pointwise_train_forward", levels, n_levels, B, Cin, Cout, 1, 1, w_dev, nullptr, nullptr, workspace_dev,
                              workspace_bytes, stream, true);
}

extern "C" int ssd_sn_pointwise_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                               const float *w_dev, float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (const char *why = sn_pw_sizes(Cin, Cout)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_sn_pointwise_train_backward: ") + why);
    return conv_train_backward("ssd_sn_pointwise_train_backward", levels, n_levels, B, Cin, Cout, 1, 1, w_dev, dw_dev, nullptr, workspace_dev,
                               workspace_bytes, stream, true, true);
}

extern "C" int ssd_sn_bn_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, int32_t training, float epsilon,
                                       float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return bn_train_forward("ssd_sn_bn_train_forward", levels, n_levels, C, act, training, epsilon, one_minus_momentum, workspace_dev,
                            workspace_bytes, stream, true);
}

extern "C" int ssd_sn_bn_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, void *workspace_dev,
                                        size_t workspace_bytes, void *stream)
{
    return bn_train_backward("ssd_sn_bn_train_backward", levels, n_levels, C, act, workspace_dev, workspace_bytes, stream, true);
}

// ----------------------------------------------------------------------------- shuffle, concat, split
// Four copies between two [rows, D] tensors a, b and either two more (p, q) or one [rows, 2D] tensor (p), V words per access
// (4: D % 4 == 0, 2: D % 2 == 0, else 1); a thread takes the words i0 .. i0 + V - 1 of a row of a and of b.  Words are moved as
// 32-bit integers: every bit pattern arrives unchanged.
//   SN_SHUFFLE    z[2i] = a[i], z[2i+1] = b[i]; p = z[:D], q = z[D:]: the thread's 2V words z[2 i0 ..] go out as two V-word stores,
//                 each wholly inside p or q (D % V == 0)
//   SN_UNSHUFFLE  its transpose: a[i] = z[2i], b[i] = z[2i+1] with z = [p | q]; a and b are written
//   SN_CONCAT     p[r, :D] = a[r], p[r, D:] = b[r]
//   SN_SPLIT      its transpose; a and b are written
enum { SN_SHUFFLE = 0, SN_UNSHUFFLE = 1, SN_CONCAT = 2, SN_SPLIT = 3 };
#define SN_COPY_MAX_BLOCKS (256 * 32)      // the grid-stride launch's block cap

template <int V, int MODE>
__global__ __launch_bounds__(256) void sn_copy_kernel(unsigned *a, unsigned *b, unsigned *p, unsigned *q, long long rows, int D)
{
    typedef unsigned vu __attribute__((ext_vector_type(V)));
    const int DV = D / V;
    const long long total = rows * DV;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int i0 = (int)(idx % DV) * V;
        const long long r = idx / DV;
        unsigned *pa = a + r * D + i0, *pb = b + r * D + i0;
        if (MODE == SN_CONCAT) {
            *(vu *)(p + r * 2 * D + i0) = *(const vu *)pa;
            *(vu *)(p + r * 2 * D + D + i0) = *(const vu *)pb;
        } else if (MODE == SN_SPLIT) {
            *(vu *)pa = *(const vu *)(p + r * 2 * D + i0);
            *(vu *)pb = *(const vu *)(p + r * 2 * D + D + i0);
        } else {
            // z words 2 i0 .. 2 i0 + V - 1 (lo) and 2 i0 + V .. 2 i0 + 2V - 1 (hi); V == 1: lo = z[2 i0], hi = z[2 i0 + 1]
            const int m0 = 2 * i0, m1 = 2 * i0 + V;
            unsigned *zlo = (m0 < D ? p + m0 : q + (m0 - D)) + r * D, *zhi = (m1 < D ? p + m1 : q + (m1 - D)) + r * D;
            unsigned z[2 * V];
            if (MODE == SN_SHUFFLE) {
                const vu va = *(const vu *)pa, vb = *(const vu *)pb;
#pragma unroll
                for (int k = 0; k < V; ++k) { z[2 * k] = ((const unsigned *)&va)[k]; z[2 * k + 1] = ((const unsigned *)&vb)[k]; }
                vu lo, hi;
#pragma unroll
                for (int k = 0; k < V; ++k) { ((unsigned *)&lo)[k] = z[k]; ((unsigned *)&hi)[k] = z[V + k]; }
                *(vu *)zlo = lo;
                *(vu *)zhi = hi;
            } else {
                const vu lo = *(const vu *)zlo, hi = *(const vu *)zhi;
#pragma unroll
                for (int k = 0; k < V; ++k) { z[k] = ((const unsigned *)&lo)[k]; z[V + k] = ((const unsigned *)&hi)[k]; }
                vu va, vb;
#pragma unroll
                for (int k = 0; k < V; ++k) { ((unsigned *)&va)[k] = z[2 * k]; ((unsigned *)&vb)[k] = z[2 * k + 1]; }
                *(vu *)pa = va;
                *(vu *)pb = vb;
            }
        }
    }
}

template <int MODE>
static hipError_t launch_sn_copy(const void *a, const void *b, const void *p, const void *q, long long rows, int D, hipStream_t s)
{
    const int V = D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1;
    const long long total = rows * (D / V);
    const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, SN_COPY_MAX_BLOCKS));
    unsigned *ua = (unsigned *)a, *ub = (unsigned *)b, *up = (unsigned *)p, *uq = (unsigned *)q;
    if (V == 4) hipLaunchKernelGGL((sn_copy_kernel<4, MODE>), grid, dim3(256), 0, s, ua, ub, up, uq, rows, D);
    else if (V == 2) hipLaunchKernelGGL((sn_copy_kernel<2, MODE>), grid, dim3(256), 0, s, ua, ub, up, uq, rows, D);
    else hipLaunchKernelGGL((sn_copy_kernel<1, MODE>), grid, dim3(256), 0, s, ua, ub, up, uq, rows, D);
    return hipGetLastError();
}

static const char *sn_copy_sizes(long long rows, int D)
{
    if (rows < 1) return "rows must be positive";
    if (D < 1 || D > (1 << 20)) return "D must be 1 .. 2^20";
    if (rows >= (1LL << 40) / D / 2) return "rows * D must stay below 2^39 elements";
    return nullptr;
}

// [p, p + n floats) of a read tensor and of a written one share a byte
static bool sn_overlap(const float *rd, long long nr, const float *wr, long long nw)
{
    return (uintptr_t)rd < (uintptr_t)(wr + nw) && (uintptr_t)wr < (uintptr_t)(rd + nr);
}

extern "C" int ssd_sn_shuffle_train(const float *x_dev, const float *y_dev, int64_t rows, int32_t D, int32_t transpose, float *xo_dev,
                                    float *yo_dev, void *stream)
{
    if (const char *why = sn_copy_sizes(rows, D)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_sn_shuffle_train: ") + why);
    if (!x_dev || !y_dev || !xo_dev || !yo_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_shuffle_train: null pointer (x_dev, y_dev, xo_dev, yo_dev)");
    if (mis16(x_dev) || mis16(y_dev) || mis16(xo_dev) || mis16(yo_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_sn_shuffle_train: every pointer needs 16-byte alignment");
    const long long n = (long long)rows * D;
    if (sn_overlap(x_dev, n, xo_dev, n) || sn_overlap(x_dev, n, yo_dev, n) || sn_overlap(y_dev, n, xo_dev, n) || sn_overlap(y_dev, n, yo_dev, n) ||
        sn_overlap(xo_dev, n, yo_dev, n))
        return ssd_fail(SSD_ERR_INVALID, "ssd_sn_shuffle_train: the inputs x_dev, y_dev and the outputs xo_dev, yo_dev must not overlap");
    // the transpose reads [p | q] = (x_dev, y_dev) and writes a, b = (xo_dev, yo_dev)
    HIPCHK(transpose ? launch_sn_copy<SN_UNSHUFFLE>(xo_dev, yo_dev, x_dev, y_dev, rows, D, (hipStream_t)stream)
                     : launch_sn_copy<SN_SHUFFLE>(x_dev, y_dev, xo_dev, yo_dev, rows, D, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" int ssd_sn_concat_train(const float *x_dev, const float *y_dev, int64_t rows, int32_t D, float *out_dev, void *stream)
{
    if (const char *why = sn_copy_sizes(rows, D)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_sn_concat_train: ") + why);
    if (!x_dev || !y_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_concat_train: null pointer (x_dev, y_dev, out_dev)");
    if (mis16(x_dev) || mis16(y_dev) || mis16(out_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_concat_train: every pointer needs 16-byte alignment");
    const long long n = (long long)rows * D;
    if (sn_overlap(x_dev, n, out_dev, 2 * n) || sn_overlap(y_dev, n, out_dev, 2 * n))
        return ssd_fail(SSD_ERR_INVALID, "ssd_sn_concat_train: x_dev, y_dev and out_dev must not overlap");
    HIPCHK(launch_sn_copy<SN_CONCAT>(x_dev, y_dev, out_dev, nullptr, rows, D, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" int ssd_sn_split_train(const float *g_dev, int64_t rows, int32_t D, float *dx_dev, float *dy_dev, void *stream)
{
    if (const char *why = sn_copy_sizes(rows, D)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_sn_split_train: ") + why);
    if (!g_dev || !dx_dev || !dy_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_split_train: null pointer (g_dev, dx_dev, dy_dev)");
    if (mis16(g_dev) || mis16(dx_dev) || mis16(dy_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_split_train: every pointer needs 16-byte alignment");
    const long long n = (long long)rows * D;
    if (sn_overlap(g_dev, 2 * n, dx_dev, n) || sn_overlap(g_dev, 2 * n, dy_dev, n) || sn_overlap(dx_dev, n, dy_dev, n))
        return ssd_fail(SSD_ERR_INVALID, "ssd_sn_split_train: g_dev, dx_dev and dy_dev must not overlap");
    HIPCHK(launch_sn_copy<SN_SPLIT>(dx_dev, dy_dev, g_dev, nullptr, rows, D, (hipStream_t)stream));
    return SSD_OK;
}

// ----------------------------------------------------------------------------- the max pool's gradient
// dx[b,iy,ix,c] = the sum of dy[b,oy,ox,c] over the windows (rows 2oy .. 2oy+2, columns 2ox .. 2ox+2, cells beyond the edge outside)
// that hold (iy,ix) and in which it is the WINNER: the first tap in row-major order whose value equals the window's output, the
// output being the forward's m = a > m ? a : m from -inf (elementwise.hip maxpool_kernel).  An input position lies in at most four
// windows (oy = iy / 2 - 1 and iy / 2 for even iy, (iy - 1) / 2 for odd iy; ox likewise): a gather, one fp32 addition per won window
// from +0 in ascending (oy, ox).  A window whose output equals none of its taps (all NaN) has no winner.
// One thread = one input position x 4 channels; it recomputes the (at most four) windows from x.
__global__ __launch_bounds__(256) void maxpool_backward_kernel(const float *__restrict__ x, const float *__restrict__ dy, int B, int H, int W, int C,
                                                                float *__restrict__ dx)
{
    const int OH = H >> 1, OW = W >> 1, C4 = C >> 2;
    const long long total = (long long)B * H * W * C4;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)(idx % C4) * 4;
        long long pix = idx / C4;
        const int ix = (int)(pix % W);
        pix /= W;
        const int iy = (int)(pix % H), b = (int)(pix / H);
        v4f g = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int oy = (iy >> 1) - ((iy & 1) ? 0 : 1); oy <= (iy >> 1); ++oy) {
            if (oy < 0) continue;
            for (int ox = (ix >> 1) - ((ix & 1) ? 0 : 1); ox <= (ix >> 1); ++ox) {
                if (ox < 0) continue;
                v4f tap[9], m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                bool in[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int ty = 2 * oy + t / 3, tx = 2 * ox + t % 3;
                    in[t] = ty < H && tx < W;
                    tap[t] = m;
                    if (in[t]) {
                        tap[t] = *(const v4f *)(x + (((long long)b * H + ty) * W + tx) * C + c);
#pragma unroll
                        for (int e = 0; e < 4; ++e) m[e] = tap[t][e] > m[e] ? tap[t][e] : m[e];
                    }
                }
                const int me = (iy - 2 * oy) * 3 + (ix - 2 * ox);
                const v4f d = *(const v4f *)(dy + (((long long)b * OH + oy) * OW + ox) * C + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int first = -1;
#pragma unroll
                    for (int t = 8; t >= 0; --t)
                        if (in[t] && tap[t][e] == m[e]) first = t;
                    if (first == me) g[e] = g[e] + d[e];
                }
            }
        }
        *(v4f *)(dx + idx * 4) = g;
    }
}

extern "C" int ssd_sn_maxpool_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C, float *dx_dev,
                                             void *stream)
{
    if (B < 1 || H < 2 || W < 2 || C < 4) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: B >= 1, H and W >= 2, C >= 4");
    if ((H & 1) || (W & 1)) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: H and W must be even");
    if (C % 4) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: C must be a multiple of 4");
    if (B > 65536 || H > 32768 || W > 32768 || (long long)B * H * W >= (1LL << 31) || (long long)B * H * W * C >= (1LL << 40))
        return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: B <= 65536, H and W <= 32768, fewer than 2^31 positions and 2^40 elements");
    if (!x_dev || !dy_dev || !dx_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: null pointer (x_dev, dy_dev, dx_dev)");
    if (mis16(x_dev) || mis16(dy_dev) || mis16(dx_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: every pointer needs 16-byte alignment");
    if (dx_dev == x_dev || dx_dev == dy_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_sn_maxpool_train_backward: dx_dev must not alias x_dev or dy_dev");
    const long long total = (long long)B * H * W * (C / 4);
    const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 256 * 64));
    LAUNCH(maxpool_backward_kernel, grid, (hipStream_t)stream, x_dev, dy_dev, B, H, W, C, dx_dev);
    return SSD_OK;
}
