// The TRAIN backbone's depthwise convolution (include/ssd_hip.h, "the TRAIN backbone"): the raw 3x3 depthwise forward on the
// caller's device weights (the inference kernel, elementwise.hip), its data gradient (one streaming kernel) and its weight gradient
// (9 * C column sums in double on the column-sum core of train_head.h, the batch norm's slab order).  The 1x1 data gradient and the
// batch norm + ReLU6 of the same header block live in train_head.hip beside the calls they extend.
// The TRAIN first convolution (the header block of that name) follows: Conv2d_0's raw forward (the inference kernels on the caller's
// device weights) and its weight gradient from the uint8 frames (27 * Cout column sums in double, the same slab order).
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`; scratch is the caller's workspace.
#include "host.h"
#include "train_head.h"
#include "first_pixels.h"

#include <algorithm>

// the plan of a depthwise call (dw_plan) and, with the pointers, the weight gradient's launch arguments
struct DwArgs {
    const float *x, *dy;
    int H, W, C, OH, OW, stride, pad;
    Slabs sl;                        // of the OUTPUT rows B * OH * OW
    double *partial;                 // [n_slabs][9][C]
};

// TF 'SAME' for a 3x3 window: out = ceil(n / stride), pad_beg = max((out - 1) * stride + 3 - n, 0) / 2
static inline int same_pad(int n, int stride) { return std::max(((n + stride - 1) / stride - 1) * stride + 3 - n, 0) / 2; }

// even_c (the TRAIN ShuffleNet's entry points): any even C, C % 4 == 2 on 8-byte accesses
static const char *dw_plan(int B, int H, int W, int C, int stride, bool backward, DwArgs &p, bool even_c = false)
{
    if (B < 1 || H < 1 || W < 1 || C < 1) return "sizes must be positive";
    if (C % (even_c ? 2 : 4)) return even_c ? "C must be even" : "C must be a multiple of 4";
    if (stride != 1 && stride != 2) return "stride must be 1 or 2";
    if (stride == 2 && ((H ^ W) & 1)) return "stride 2 needs H and W of the same parity (one pad_beg for both axes)";
    if (B > 65536 || H > 32768 || W > 32768 || (long long)B * H * W >= (1LL << 31) || (long long)B * H * W * C >= (1LL << 40))
        return "B <= 65536, H and W <= 32768, fewer than 2^31 positions and 2^40 elements";
    if (backward && C > 1024) return "the backward takes at most 1024 channels";
    p.H = H; p.W = W; p.C = C; p.stride = stride;
    p.OH = (H + stride - 1) / stride;
    p.OW = (W + stride - 1) / stride;
    p.pad = same_pad(H, stride);
    p.sl = slab_rule((long long)B * p.OH * p.OW, (std::min(C, TH_STAT_COLS) + 3) / 4);   // (the forward takes wider tensors; it has no slabs)
    return nullptr;
}

static size_t dw_bytes(const DwArgs &p) { return al256((size_t)p.sl.n_slabs * 9 * p.C * 8); }

// ----------------------------------------------------------------------------- the data gradient
// dx[b,iy,ix,c] = sum over the taps (ky,kx) of dy[b,(iy+P-ky)/S,(ix+P-kx)/S,c] * w[ky,kx,c] whose source index is an integer inside
// the output: ONE fmaf chain per element from +0 over ky = 2, 1, 0 and within each kx = 2, 1, 0, taps without a source skipped.
// One thread = 2 rows x 4 pixels of dx x V channels (V = 4, or 2 where C % 4 == 2: 8-byte accesses).  The dy rows it needs (4 rows x 6 pixels at stride 1, 2 x 3 at stride 2, where
// every dy value serves up to four dx pixels) are streamed top to bottom, each loaded once; a dy row further down is a tap row
// further up (ky smaller), so every element still sees its taps in the pinned order.  S and P (pad_beg) are template arguments and
// a tile starts on even coordinates, so which tap meets which window cell is decided at compile time.
template <int S, int P, int V = 4>
__global__ __launch_bounds__(256) void dw_dx_kernel(const float *__restrict__ dy, int B, int H, int W, int C, const float *__restrict__ w,
                                                     int OH, int OW, float *__restrict__ dx)
{
    constexpr int TR = 2, TC = 4;
    constexpr int NWR = S == 1 ? TR + 2 : TR / 2 + 1, NWC = S == 1 ? TC + 2 : TC / 2 + 1;
    constexpr int OFF = S == 1 ? P - 2 : (P == 0 ? -1 : 0);             // first source index of a tile at i0: i0 / S + OFF
    typedef float vf __attribute__((ext_vector_type(V)));
    const int C4 = C >> (V == 4 ? 2 : 1), XG = (W + TC - 1) / TC, YG = (H + TR - 1) / TR;
    const long long total = (long long)B * YG * XG * C4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4) * V;
        long long q = idx / C4;
        const int ix0 = (int)(q % XG) * TC;
        q /= XG;
        const int iy0 = (int)(q % YG) * TR;
        const int b = (int)(q / YG);
        const int oy0 = iy0 / S + OFF, ox0 = ix0 / S + OFF;
        vf wv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wv[t] = *(const vf *)(w + t * C + c);
        vf acc[TR][TC];
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int p = 0; p < TC; ++p) acc[r][p] = (vf)(0.0f);
#pragma unroll
        for (int j = 0; j < NWR; ++j) {
            const int oy = oy0 + j;
            const bool rowok = (unsigned)oy < (unsigned)OH;
            const float *rowp = dy + (((long long)b * OH + (rowok ? oy : 0)) * OW) * C + c;
            vf d[NWC];
            bool ok[NWC];
#pragma unroll
            for (int k = 0; k < NWC; ++k) {
                const int ox = ox0 + k;
                ok[k] = rowok && (unsigned)ox < (unsigned)OW;
                d[k] = (vf)(0.0f);
                if (ok[k]) d[k] = *(const vf *)(rowp + (long long)ox * C);
            }
#pragma unroll
            for (int r = 0; r < TR; ++r) {
#pragma unroll
                for (int jy = 0; jy < 3; ++jy) {                         // tap row ky = 2 - jy of dx row r
                    const int vy = r + P - (2 - jy);
                    if ((S == 2 && (vy & 1)) || (S == 1 ? vy : vy / 2) - OFF != j) continue;
#pragma unroll
                    for (int p = 0; p < TC; ++p) {
#pragma unroll
                        for (int jx = 0; jx < 3; ++jx) {
                            const int vx = p + P - (2 - jx);
                            if (S == 2 && (vx & 1)) continue;
                            const int k = (S == 1 ? vx : vx / 2) - OFF;
                            if (ok[k]) {
#pragma unroll
                                for (int i = 0; i < V; ++i) acc[r][p][i] = fmaf(d[k][i], wv[(2 - jy) * 3 + (2 - jx)][i], acc[r][p][i]);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (iy0 + r >= H) continue;
            float *o = dx + (((long long)b * H + iy0 + r) * W + ix0) * C + c;
#pragma unroll
            for (int p = 0; p < TC; ++p)
                if (ix0 + p < W) *(vf *)(o + (long long)p * C) = acc[r][p];
        }
    }
}

// ----------------------------------------------------------------------------- the weight gradient
// The column-sum core of train_head.h over the output rows, G = ceil(C / 4) (VW: th_load4's access width, 4 or -- C % 4 == 2 -- 2,
// the second pair of the last quad then lies outside and stays +0): a thread keeps the nine taps' sums of x * dy of its channel
// quad in double (the product of two floats is exact in double); the block then adds its row lanes one tap at a time.
template <int VW>
__global__ __launch_bounds__(256) void dw_wgrad_partial(const DwArgs a)
{
    __shared__ double sm[1024];
    const int tid = threadIdx.x, slab = blockIdx.x;
    const int C = a.C, G = (C + 3) >> 2;
    const SlabLane ln = slab_lane(tid, G, slab, a.sl.slab_rows, a.sl.R);
    const int c = ln.c;
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
    if (ln.on) {
        for (long long r = ln.r0 + ln.rl; r < ln.r1; r += ln.rpp) {
            const unsigned ur = (unsigned)r;
            const int ox = (int)(ur % (unsigned)a.OW);
            const unsigned qq = ur / (unsigned)a.OW;
            const int oy = (int)(qq % (unsigned)a.OH), b = (int)(qq / (unsigned)a.OH);
            const v4f d = th_load4(a.dy + r * C, c, C, VW);
            const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = iy0 + ky;
                if ((unsigned)iy >= (unsigned)a.H) continue;
                const float *rowp = a.x + (((long long)b * a.H + iy) * a.W) * C + c;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ix0 + kx;
                    if ((unsigned)ix >= (unsigned)a.W) continue;
                    const v4f xv = th_load4(rowp + (long long)ix * C - c, c, C, VW);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[ky * 3 + kx][e] += (double)xv[e] * (double)d[e];
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        slab_reduce4(sm, acc[t], tid, G, a.partial + ((long long)slab * 9 + t) * C, 0, C);
        __syncthreads();                                     // sm goes round again
    }
}

// ----------------------------------------------------------------------------- entry points
// the bodies (train_head.h): even_c is the TRAIN ShuffleNet's flag; without it the arguments, refusals, launches and bits of before
int dw_train_forward(const std::string &fn, const float *x_dev, int B, int H, int W, int C, const float *w_dev, int stride, float *out_dev,
                     void *stream, bool even_c)
{
    DwArgs p;
    if (const char *why = dw_plan(B, H, W, C, stride, false, p, even_c)) return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (!x_dev || !w_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, fn + ": null pointer");
    if (mis16(x_dev) || mis16(w_dev) || mis16(out_dev)) return ssd_fail(SSD_ERR_INVALID, fn + ": every pointer needs 16-byte alignment");
    HIPCHK(launch_depthwise(x_dev, B, H, W, C, w_dev, stride, p.pad, p.OH, p.OW, nullptr, nullptr, nullptr, SSD_ACT_NONE, out_dev, (hipStream_t)stream, 0,
                            nullptr, C % 4 ? 1 : 0));
    return SSD_OK;
}

size_t dw_train_workspace(int B, int H, int W, int C, int stride, bool even_c)
{
    DwArgs p;
    return dw_plan(B, H, W, C, stride, true, p, even_c) ? 0 : dw_bytes(p);
}

template <int V>
static hipError_t launch_dw_backward(const DwArgs &a, int B, const float *w_dev, float *dx_dev, hipStream_t s)
{
    if (dx_dev) {
        const long long total = (long long)B * ((a.H + 1) / 2) * ((a.W + 3) / 4) * (a.C / V);
        const unsigned blocks = (unsigned)std::max(1LL, std::min<long long>((total + 255) / 256, 256 * 64));
        if (a.stride == 1)
            hipLaunchKernelGGL((dw_dx_kernel<1, 1, V>), dim3(blocks), dim3(256), 0, s, a.dy, B, a.H, a.W, a.C, w_dev, a.OH, a.OW, dx_dev);
        else if (a.pad == 0)
            hipLaunchKernelGGL((dw_dx_kernel<2, 0, V>), dim3(blocks), dim3(256), 0, s, a.dy, B, a.H, a.W, a.C, w_dev, a.OH, a.OW, dx_dev);
        else
            hipLaunchKernelGGL((dw_dx_kernel<2, 1, V>), dim3(blocks), dim3(256), 0, s, a.dy, B, a.H, a.W, a.C, w_dev, a.OH, a.OW, dx_dev);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(dw_wgrad_partial<V>, dim3((unsigned)a.sl.n_slabs), dim3(256), 0, s, a);
    return hipGetLastError();
}

int dw_train_backward(const std::string &fn, const float *x_dev, const float *dy_dev, int B, int H, int W, int C, const float *w_dev, int stride,
                      float *dx_dev, float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream, bool even_c)
{
    DwArgs a;
    if (const char *why = dw_plan(B, H, W, C, stride, true, a, even_c)) return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (!x_dev || !dy_dev || !w_dev || !dw_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, fn + ": null pointer");
    if (mis16(x_dev) || mis16(dy_dev) || mis16(w_dev) || mis16(dx_dev) || mis16(dw_dev) || mis16(workspace_dev))
        return ssd_fail(SSD_ERR_INVALID, fn + ": every pointer needs 16-byte alignment");
    if (workspace_bytes < dw_bytes(a)) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    a.x = x_dev; a.dy = dy_dev;
    a.partial = (double *)workspace_dev;
    HIPCHK(C % 4 ? launch_dw_backward<2>(a, B, w_dev, dx_dev, s) : launch_dw_backward<4>(a, B, w_dev, dx_dev, s));
    HIPCHK(launch_slab_sum(a.partial, a.sl.n_slabs, 9LL * C, 9 * C, dw_dev, s));
    return SSD_OK;
}

extern "C" int ssd_depthwise_train_forward(const float *x_dev, int32_t B, int32_t H, int32_t W, int32_t C, const float *w_dev,
                                           int32_t stride, float *out_dev, void *stream)
{
    return dw_train_forward("ssd_depthwise_train_forward", x_dev, B, H, W, C, w_dev, stride, out_dev, stream, false);
}

extern "C" size_t ssd_depthwise_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride)
{
    return dw_train_workspace(B, H, W, C, stride, false);
}

extern "C" int ssd_depthwise_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                                            const float *w_dev, int32_t stride, float *dx_dev, float *dw_dev, void *workspace_dev,
                                            size_t workspace_bytes, void *stream)
{
    return dw_train_backward("ssd_depthwise_train_backward", x_dev, dy_dev, B, H, W, C, w_dev, stride, dx_dev, dw_dev, workspace_dev, workspace_bytes,
                             stream, false);
}

// ============================================================================= the TRAIN first convolution
// the plan of a first-convolution call (fc_plan) and, with the pointers, the weight gradient's launch arguments
struct FcArgs {
    const uint8_t *img;
    const float *dy;
    int B, H, W, C, OH, OW;          // C = Cout
    Slabs sl;                        // of the OUTPUT rows B * OH * OW
    double *partial;                 // [n_slabs][27][C]
};

static const char *fc_plan(int B, int H, int W, int Cout, FcArgs &p)
{
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be positive";
    if ((H & 1) || (W & 1)) return "H and W must be even (the network's own size)";
    if (Cout < 4 || Cout > 64 || Cout % 4) return "Cout must be a multiple of 4 and at most 64";
    if ((long long)B * H * W * 3 >= (1LL << 31)) return "B * H * W * 3 must stay below 2^31";
    p.B = B; p.H = H; p.W = W; p.C = Cout;
    p.OH = H / 2;
    p.OW = W / 2;
    p.sl = slab_rule((long long)B * p.OH * p.OW, Cout / 4);
    return nullptr;
}

static size_t fc_bytes(const FcArgs &p) { return al256((size_t)p.sl.n_slabs * 27 * p.C * 8); }

// dw_wgrad_partial's sibling.  Block = slab of output rows x the three filter rows: thread (ky = threadIdx.y, tid = threadIdx.x)
// is lane tid of the column-sum core, G = C / 4, for filter row ky: it keeps the sums of p * dy of that row -- 3 pixels x 3
// channels x 4 output channels, 36 doubles -- so that the 27 x 4 accumulators of a channel quad are spread over three threads of
// one block, which read the same dy rows at about the same time, instead of filling one thread's register file.  The nine bytes
// under a filter row come from fc_row_fetch / fc_row_bytes and their values from fc_pixel (first_pixels.h), as in the forward
// kernels.  Only row 2oy+2 and column 2ox+2 can lie outside the image: such taps are skipped.  The product of two
// floats is exact in double, so fma(p, dy, acc) has the bits of acc + p * dy.  The block then adds its row lanes one tap at a
// time, each filter row in its own third of the LDS.
__global__ __launch_bounds__(768) void fc_wgrad_partial(const FcArgs a)
{
    __shared__ double sm[3][1024];
    const int tid = threadIdx.x, ky = threadIdx.y, slab = blockIdx.x;
    const int C = a.C, G = C >> 2;
    const SlabLane ln = slab_lane(tid, G, slab, a.sl.slab_rows, a.sl.R);
    const int c = ln.c, rpp = ln.rpp;
    const long long r0 = ln.r0, r1 = ln.r1;
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.img, 0, (int)((long long)a.B * a.H * a.W * 3), 0x00020000);
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
    if (ln.on) {
        // r -> (row = b * OH + oy, ox) once; a step of rpp rows then moves ox by rpp % OW and row by rpp / OW (+ 1 on a carry), and
        // oy = row % OH follows with one conditional subtraction: no division inside the loop.  H = 2 * OH, so the image row of
        // tap ky is b * H + 2 * oy + ky = 2 * row + ky.
        const int OW = a.OW, OH = a.OH;
        const int step_x = rpp % OW, step_row = rpp / OW, step_y = step_row % OH;
        const unsigned first = (unsigned)(r0 + ln.rl);
        int ox = (int)(first % (unsigned)OW), row = (int)(first / (unsigned)OW), oy = row % OH;
        for (long long r = r0 + ln.rl; r < r1; r += rpp) {
            const int cx = ox, crow = row, cy = oy;
            ox += step_x; row += step_row; oy += step_y;
            if (ox >= OW) { ox -= OW; ++row; ++oy; }
            if (oy >= OH) oy -= OH;
            if (ky == 2 && cy == OH - 1) continue;           // row H: outside
            const v4f d = *(const v4f *)(a.dy + r * C + c);
            const double dd[4] = {(double)d[0], (double)d[1], (double)d[2], (double)d[3]};
            const int ad = ((2 * crow + ky) * a.W + 2 * cx) * 3;
            unsigned w0, w1, w2;
            unsigned char px[9];
            fc_row_fetch<true>(irsrc, true, ad, w0, w1, w2);
            fc_row_bytes(w0, w1, w2, ad & 3, px);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double pv = (double)fc_pixel(px[k]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k][e] = fma(pv, dd[e], acc[k][e]);
            }
            if (cx < OW - 1) {                               // else column W: outside
#pragma unroll
                for (int k = 6; k < 9; ++k) {
                    const double pv = (double)fc_pixel(px[k]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[k][e] = fma(pv, dd[e], acc[k][e]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        slab_reduce4(sm[ky], acc[t], tid, G, a.partial + ((long long)slab * 27 + ky * 9 + t) * C, 0, C);
        __syncthreads();                                     // sm goes round again
    }
}

extern "C" int ssd_first_conv_train_forward(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W, const float *w_dev, int32_t Cout,
                                            float *out_dev, void *stream)
{
    FcArgs p;
    if (const char *why = fc_plan(B, H, W, Cout, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_train_forward: ") + why);
    if (!images_dev || !w_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: null pointer (images_dev, w_dev, out_dev)");
    if (mis16(w_dev) || mis16(out_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: w_dev and out_dev need 16-byte alignment");
    if ((uintptr_t)images_dev & 3) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: images_dev needs 4-byte alignment");
    HIPCHK(launch_first_conv(images_dev, B, H, W, H, W, H, W, w_dev, Cout, nullptr, nullptr, nullptr, SSD_ACT_NONE, out_dev, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" size_t ssd_first_conv_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout)
{
    FcArgs p;
    return fc_plan(B, H, W, Cout, p) ? 0 : fc_bytes(p);
}

extern "C" int ssd_first_conv_train_backward(const uint8_t *images_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t Cout,
                                             float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    FcArgs a;
    if (const char *why = fc_plan(B, H, W, Cout, a)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_train_backward: ") + why);
    if (!images_dev || !dy_dev || !dw_dev || !workspace_dev)
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: null pointer (images_dev, dy_dev, dw_dev, workspace_dev)");
    if (mis16(dy_dev) || mis16(dw_dev) || mis16(workspace_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: dy_dev, dw_dev and workspace_dev need 16-byte alignment");
    if ((uintptr_t)images_dev & 3) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: images_dev needs 4-byte alignment");
    if (workspace_bytes < fc_bytes(a)) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    a.img = images_dev; a.dy = dy_dev;
    a.partial = (double *)workspace_dev;
    hipLaunchKernelGGL(fc_wgrad_partial, dim3((unsigned)a.sl.n_slabs), dim3(256, 3), 0, s, a);     // 256 x 3: not LAUNCH's block
    HIPCHK(hipGetLastError());
    HIPCHK(launch_slab_sum(a.partial, a.sl.n_slabs, 27LL * Cout, 27 * Cout, dw_dev, s));
    return SSD_OK;
}
