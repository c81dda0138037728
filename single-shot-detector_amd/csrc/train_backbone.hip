// The TRAIN backbone's depthwise convolution (include/ssd_hip.h, "the TRAIN backbone"): the raw 3x3 depthwise forward on the
// caller's device weights (the inference kernel, elementwise.hip), its data gradient (one streaming kernel) and its weight gradient
// (9 * C column sums in double, the two-stage slab order of the batch norm's column statistics).  The 1x1 data gradient and the
// batch norm + ReLU6 of the same header block live in train_head.hip beside the calls they extend.
// The TRAIN first convolution (the header block of that name) follows: Conv2d_0's raw forward (the inference kernels on the caller's
// device weights) and its weight gradient from the uint8 frames (27 * Cout column sums in double, the same slab order).
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`; scratch is the caller's workspace.
#include "host.h"

#include <algorithm>

typedef float v4f __attribute__((ext_vector_type(4)));

static inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
static inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

struct DwPlan {
    int OH, OW, pad;
    long long R;                     // output rows B * OH * OW
    int slab_rows, n_slabs;
    size_t bytes;
};

// TF 'SAME' for a 3x3 window: out = ceil(n / stride), pad_beg = max((out - 1) * stride + 3 - n, 0) / 2
static inline int same_pad(int n, int stride) { return std::max(((n + stride - 1) / stride - 1) * stride + 3 - n, 0) / 2; }

// The batch norm's slab rule (train_head.hip make_slabs) for R rows of C channels: slab_rows = max(8 * rpp, ceil(R / 1024)) rounded
// up to a multiple of rpp = 256 / (C / 4).
static void slab_rule(long long R, int C, int &slab_rows, int &n_slabs)
{
    const int G = C / 4, rpp = 256 / (G < 1 ? 1 : (G > 256 ? 256 : G));
    long long sr = (R + 1023) / 1024;
    if (sr < 8LL * rpp) sr = 8LL * rpp;
    sr = (sr + rpp - 1) / rpp * rpp;
    slab_rows = (int)sr;
    n_slabs = (int)((R + sr - 1) / sr);
}

static const char *dw_plan(int B, int H, int W, int C, int stride, bool backward, DwPlan &p)
{
    if (B < 1 || H < 1 || W < 1 || C < 1) return "sizes must be positive";
    if (C % 4) return "C must be a multiple of 4";
    if (stride != 1 && stride != 2) return "stride must be 1 or 2";
    if (stride == 2 && ((H ^ W) & 1)) return "stride 2 needs H and W of the same parity (one pad_beg for both axes)";
    if (B > 65536 || H > 32768 || W > 32768 || (long long)B * H * W >= (1LL << 31) || (long long)B * H * W * C >= (1LL << 40))
        return "B <= 65536, H and W <= 32768, fewer than 2^31 positions and 2^40 elements";
    if (backward && C > 1024) return "the backward takes at most 1024 channels";
    p.OH = (H + stride - 1) / stride;
    p.OW = (W + stride - 1) / stride;
    p.pad = same_pad(H, stride);
    p.R = (long long)B * p.OH * p.OW;
    slab_rule(p.R, C, p.slab_rows, p.n_slabs);                          // over the OUTPUT rows
    p.bytes = al256((size_t)p.n_slabs * 9 * C * 8);
    return nullptr;
}

// ----------------------------------------------------------------------------- the data gradient
// dx[b,iy,ix,c] = sum over the taps (ky,kx) of dy[b,(iy+P-ky)/S,(ix+P-kx)/S,c] * w[ky,kx,c] whose source index is an integer inside
// the output: ONE fmaf chain per element from +0 over ky = 2, 1, 0 and within each kx = 2, 1, 0, taps without a source skipped.
// One thread = 2 rows x 4 pixels of dx x 4 channels.  The dy rows it needs (4 rows x 6 pixels at stride 1, 2 x 3 at stride 2, where
// every dy value serves up to four dx pixels) are streamed top to bottom, each loaded once; a dy row further down is a tap row
// further up (ky smaller), so every element still sees its taps in the pinned order.  S and P (pad_beg) are template arguments and
// a tile starts on even coordinates, so which tap meets which window cell is decided at compile time.
template <int S, int P>
__global__ __launch_bounds__(256) void dw_dx_kernel(const float *__restrict__ dy, int B, int H, int W, int C, const float *__restrict__ w,
                                                     int OH, int OW, float *__restrict__ dx)
{
    constexpr int TR = 2, TC = 4;
    constexpr int NWR = S == 1 ? TR + 2 : TR / 2 + 1, NWC = S == 1 ? TC + 2 : TC / 2 + 1;
    constexpr int OFF = S == 1 ? P - 2 : (P == 0 ? -1 : 0);             // first source index of a tile at i0: i0 / S + OFF
    const int C4 = C >> 2, XG = (W + TC - 1) / TC, YG = (H + TR - 1) / TR;
    const long long total = (long long)B * YG * XG * C4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4) * 4;
        long long q = idx / C4;
        const int ix0 = (int)(q % XG) * TC;
        q /= XG;
        const int iy0 = (int)(q % YG) * TR;
        const int b = (int)(q / YG);
        const int oy0 = iy0 / S + OFF, ox0 = ix0 / S + OFF;
        v4f wv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wv[t] = *(const v4f *)(w + t * C + c);
        v4f acc[TR][TC];
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int p = 0; p < TC; ++p) acc[r][p] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < NWR; ++j) {
            const int oy = oy0 + j;
            const bool rowok = (unsigned)oy < (unsigned)OH;
            const float *rowp = dy + (((long long)b * OH + (rowok ? oy : 0)) * OW) * C + c;
            v4f d[NWC];
            bool ok[NWC];
#pragma unroll
            for (int k = 0; k < NWC; ++k) {
                const int ox = ox0 + k;
                ok[k] = rowok && (unsigned)ox < (unsigned)OW;
                d[k] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
                if (ok[k]) d[k] = *(const v4f *)(rowp + (long long)ox * C);
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
                                for (int i = 0; i < 4; ++i) acc[r][p][i] = fmaf(d[k][i], wv[(2 - jy) * 3 + (2 - jx)][i], acc[r][p][i]);
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
                if (ix0 + p < W) *(v4f *)(o + (long long)p * C) = acc[r][p];
        }
    }
}

// ----------------------------------------------------------------------------- the weight gradient
struct DwGradArgs {
    const float *x, *dy;
    int H, W, C, OH, OW, stride, pad;
    long long R;
    int slab_rows, n_slabs;
    double *partial;                 // [n_slabs][9][C]
};

// Block = slab of output rows; thread (rl = tid / G, g = tid % G), G = C / 4, rpp = 256 / G, walks the rows r0 + rl, r0 + rl + rpp, ...
// of its slab for the channel quad g and keeps the nine taps' sums of x * dy in double (the product of two floats is exact in
// double); the block then adds its rpp row lanes in ascending order, one tap at a time through LDS.
__global__ __launch_bounds__(256) void dw_wgrad_partial(const DwGradArgs a)
{
    __shared__ double sm[1024];
    const int tid = threadIdx.x, slab = blockIdx.x;
    const int C = a.C, G = C >> 2, rpp = 256 / G;
    const int rl = tid / G, g = tid - rl * G, c = g << 2;
    const long long r0 = (long long)slab * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < a.R ? r0 + a.slab_rows : a.R;
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
    if (rl < rpp) {
        for (long long r = r0 + rl; r < r1; r += rpp) {
            const unsigned ur = (unsigned)r;
            const int ox = (int)(ur % (unsigned)a.OW);
            const unsigned qq = ur / (unsigned)a.OW;
            const int oy = (int)(qq % (unsigned)a.OH), b = (int)(qq / (unsigned)a.OH);
            const v4f d = *(const v4f *)(a.dy + r * C + c);
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
                    const v4f xv = *(const v4f *)(rowp + (long long)ix * C);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[ky * 3 + kx][e] += (double)xv[e] * (double)d[e];
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sm[tid * 4 + e] = acc[t][e];
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = 0.0;
                for (int j = 0; j < rpp; ++j) s += sm[(j * G + g) * 4 + e];
                a.partial[((long long)slab * 9 + t) * C + c + e] = s;
            }
        }
        __syncthreads();
    }
}

// dw[t][c] = fp32(the slabs' sums added in ascending order)
__global__ __launch_bounds__(256) void dw_wgrad_final(const DwGradArgs a, float *dw)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9 * a.C) return;
    double s = 0.0;
    for (int k = 0; k < a.n_slabs; ++k) s += a.partial[(long long)k * 9 * a.C + idx];
    dw[idx] = (float)s;
}

// ----------------------------------------------------------------------------- entry points
extern "C" int ssd_depthwise_train_forward(const float *x_dev, int32_t B, int32_t H, int32_t W, int32_t C, const float *w_dev,
                                           int32_t stride, float *out_dev, void *stream)
{
    DwPlan p;
    if (const char *why = dw_plan(B, H, W, C, stride, false, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_depthwise_train_forward: ") + why);
    if (!x_dev || !w_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_depthwise_train_forward: null pointer");
    if (mis16(x_dev) || mis16(w_dev) || mis16(out_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_depthwise_train_forward: every pointer needs 16-byte alignment");
    HIPCHK(launch_depthwise(x_dev, B, H, W, C, w_dev, stride, p.pad, p.OH, p.OW, nullptr, nullptr, nullptr, SSD_ACT_NONE, out_dev, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" size_t ssd_depthwise_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride)
{
    DwPlan p;
    return dw_plan(B, H, W, C, stride, true, p) ? 0 : p.bytes;
}

extern "C" int ssd_depthwise_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                                            const float *w_dev, int32_t stride, float *dx_dev, float *dw_dev, void *workspace_dev,
                                            size_t workspace_bytes, void *stream)
{
    DwPlan p;
    if (const char *why = dw_plan(B, H, W, C, stride, true, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_depthwise_train_backward: ") + why);
    if (!x_dev || !dy_dev || !w_dev || !dw_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_depthwise_train_backward: null pointer");
    if (mis16(x_dev) || mis16(dy_dev) || mis16(w_dev) || mis16(dx_dev) || mis16(dw_dev) || mis16(workspace_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_depthwise_train_backward: every pointer needs 16-byte alignment");
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, "ssd_depthwise_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (dx_dev) {
        const long long total = (long long)B * ((H + 1) / 2) * ((W + 3) / 4) * (C / 4);
        const unsigned blocks = (unsigned)std::max(1LL, std::min<long long>((total + 255) / 256, 256 * 64));
        if (stride == 1)
            hipLaunchKernelGGL((dw_dx_kernel<1, 1>), dim3(blocks), dim3(256), 0, s, dy_dev, B, H, W, C, w_dev, p.OH, p.OW, dx_dev);
        else if (p.pad == 0)
            hipLaunchKernelGGL((dw_dx_kernel<2, 0>), dim3(blocks), dim3(256), 0, s, dy_dev, B, H, W, C, w_dev, p.OH, p.OW, dx_dev);
        else
            hipLaunchKernelGGL((dw_dx_kernel<2, 1>), dim3(blocks), dim3(256), 0, s, dy_dev, B, H, W, C, w_dev, p.OH, p.OW, dx_dev);
        HIPCHK(hipGetLastError());
    }
    DwGradArgs a;
    a.x = x_dev; a.dy = dy_dev;
    a.H = H; a.W = W; a.C = C; a.OH = p.OH; a.OW = p.OW; a.stride = stride; a.pad = p.pad;
    a.R = p.R; a.slab_rows = p.slab_rows; a.n_slabs = p.n_slabs;
    a.partial = (double *)workspace_dev;
    hipLaunchKernelGGL(dw_wgrad_partial, dim3((unsigned)p.n_slabs), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(dw_wgrad_final, dim3((unsigned)((9 * C + 255) / 256)), dim3(256), 0, s, a, dw_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

// ============================================================================= the TRAIN first convolution
struct FcPlan {
    int OH, OW;
    long long R;                     // output rows B * OH * OW
    int slab_rows, n_slabs;
    size_t bytes;
};

static const char *fc_plan(int B, int H, int W, int Cout, FcPlan &p)
{
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be positive";
    if ((H & 1) || (W & 1)) return "H and W must be even (the network's own size)";
    if (Cout < 4 || Cout > 64 || Cout % 4) return "Cout must be a multiple of 4 and at most 64";
    if ((long long)B * H * W * 3 >= (1LL << 31)) return "B * H * W * 3 must stay below 2^31";
    p.OH = H / 2;
    p.OW = W / 2;
    p.R = (long long)B * p.OH * p.OW;
    slab_rule(p.R, Cout, p.slab_rows, p.n_slabs);                       // over the OUTPUT rows, C = Cout
    p.bytes = al256((size_t)p.n_slabs * 27 * Cout * 8);
    return nullptr;
}

struct FcGradArgs {
    const uint8_t *img;
    const float *dy;
    int B, H, W, C, OH, OW;          // C = Cout
    long long R;
    int slab_rows, n_slabs;
    double *partial;                 // [n_slabs][27][C]
};

// dw_wgrad_partial's sibling.  Block = slab of output rows x the three filter rows: thread (ky = threadIdx.y, rl = tid / G,
// g = tid % G), G = C / 4, rpp = 256 / G, walks the rows r0 + rl, r0 + rl + rpp, ... of its slab for the channel quad g and keeps
// the sums of p * dy of filter row ky -- 3 pixels x 3 channels x 4 output channels, 36 doubles -- so that the 27 x 4 accumulators
// of a channel quad are spread over three threads of one block, which read the same dy rows at about the same time, instead of
// filling one thread's register file.  The nine bytes under a filter row are contiguous, 0 or 2 bytes past a dword
// boundary (W is even; which of the two depends on the row when W % 4 == 2): three aligned dword loads through a range-checked
// buffer resource and a byte alignment, as in first_conv_px_kernel (elementwise.hip).  Only row 2oy+2 and column 2ox+2 can lie
// outside the image: such taps are skipped.  The product of two floats is exact in double, so fma(p, dy, acc) has the bits of
// acc + p * dy.  The block then adds its rpp row lanes in ascending order, one tap at a time
// through LDS.
__global__ __launch_bounds__(768) void fc_wgrad_partial(const FcGradArgs a)
{
    __shared__ double sm[3][1024];
    const int tid = threadIdx.x, ky = threadIdx.y, slab = blockIdx.x;
    const int C = a.C, G = C >> 2, rpp = 256 / G;
    const int rl = tid / G, g = tid - rl * G, c = g << 2;
    const long long r0 = (long long)slab * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < a.R ? r0 + a.slab_rows : a.R;
    const float inv255 = (float)(1.0 / 255.0);
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.img, 0, (int)((long long)a.B * a.H * a.W * 3), 0x00020000);
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
    if (rl < rpp) {
        // r -> (row = b * OH + oy, ox) once; a step of rpp rows then moves ox by rpp % OW and row by rpp / OW (+ 1 on a carry), and
        // oy = row % OH follows with one conditional subtraction: no division inside the loop.  H = 2 * OH, so the image row of
        // tap ky is b * H + 2 * oy + ky = 2 * row + ky.
        const int OW = a.OW, OH = a.OH;
        const int step_x = rpp % OW, step_row = rpp / OW, step_y = step_row % OH;
        const unsigned first = (unsigned)(r0 + rl);
        int ox = (int)(first % (unsigned)OW), row = (int)(first / (unsigned)OW), oy = row % OH;
        for (long long r = r0 + rl; r < r1; r += rpp) {
            const int cx = ox, crow = row, cy = oy;
            ox += step_x; row += step_row; oy += step_y;
            if (ox >= OW) { ox -= OW; ++row; ++oy; }
            if (oy >= OH) oy -= OH;
            if (ky == 2 && cy == OH - 1) continue;           // row H: outside
            const v4f d = *(const v4f *)(a.dy + r * C + c);
            const double dd[4] = {(double)d[0], (double)d[1], (double)d[2], (double)d[3]};
            const int ad = ((2 * crow + ky) * a.W + 2 * cx) * 3;
            const int a0 = ad & ~3, sh = ad & 3;         // sh: byte offset of the row's first pixel inside its dword (0 or 2)
            const unsigned w0 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0, 0, 0);
            const unsigned w1 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0 + 4, 0, 0);
            const unsigned w2 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0 + 8, 0, 0);
            const unsigned d0 = __builtin_amdgcn_alignbyte(w1, w0, sh);
            const unsigned d1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
            const unsigned d2 = w2 >> (8 * sh);
            const unsigned char px[9] = {(unsigned char)d0, (unsigned char)(d0 >> 8), (unsigned char)(d0 >> 16), (unsigned char)(d0 >> 24),
                                         (unsigned char)d1, (unsigned char)(d1 >> 8), (unsigned char)(d1 >> 16), (unsigned char)(d1 >> 24),
                                         (unsigned char)d2};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                float v = (float)px[k] * inv255;
                v = 2.0f * v - 1.0f;
                const double pv = (double)v;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k][e] = fma(pv, dd[e], acc[k][e]);
            }
            if (cx < OW - 1) {                               // else column W: outside
#pragma unroll
                for (int k = 6; k < 9; ++k) {
                    float v = (float)px[k] * inv255;
                    v = 2.0f * v - 1.0f;
                    const double pv = (double)v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[k][e] = fma(pv, dd[e], acc[k][e]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sm[ky][tid * 4 + e] = acc[t][e];
        __syncthreads();
        if (rl < 4) {                                        // rpp >= 16: row lanes 0 .. 3 exist; lane rl adds element e = rl of the quad
            double s = 0.0;
            for (int j = 0; j < rpp; ++j) s += sm[ky][(j * G + g) * 4 + rl];
            a.partial[((long long)slab * 27 + ky * 9 + t) * C + c + rl] = s;
        }
        __syncthreads();
    }
}

// dw[t][c] = fp32(the slabs' sums added in ascending order)
__global__ __launch_bounds__(256) void fc_wgrad_final(const FcGradArgs a, float *dw)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 27 * a.C) return;
    double s = 0.0;
    for (int k = 0; k < a.n_slabs; ++k) s += a.partial[(long long)k * 27 * a.C + idx];
    dw[idx] = (float)s;
}

extern "C" int ssd_first_conv_train_forward(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W, const float *w_dev, int32_t Cout,
                                            float *out_dev, void *stream)
{
    FcPlan p;
    if (const char *why = fc_plan(B, H, W, Cout, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_train_forward: ") + why);
    if (!images_dev || !w_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: null pointer (images_dev, w_dev, out_dev)");
    if (mis16(w_dev) || mis16(out_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: w_dev and out_dev need 16-byte alignment");
    if ((uintptr_t)images_dev & 3) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_forward: images_dev needs 4-byte alignment");
    HIPCHK(launch_first_conv(images_dev, B, H, W, H, W, H, W, w_dev, Cout, nullptr, nullptr, nullptr, SSD_ACT_NONE, out_dev, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" size_t ssd_first_conv_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout)
{
    FcPlan p;
    return fc_plan(B, H, W, Cout, p) ? 0 : p.bytes;
}

extern "C" int ssd_first_conv_train_backward(const uint8_t *images_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t Cout,
                                             float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    FcPlan p;
    if (const char *why = fc_plan(B, H, W, Cout, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_train_backward: ") + why);
    if (!images_dev || !dy_dev || !dw_dev || !workspace_dev)
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: null pointer (images_dev, dy_dev, dw_dev, workspace_dev)");
    if (mis16(dy_dev) || mis16(dw_dev) || mis16(workspace_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: dy_dev, dw_dev and workspace_dev need 16-byte alignment");
    if ((uintptr_t)images_dev & 3) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: images_dev needs 4-byte alignment");
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    FcGradArgs a;
    a.img = images_dev; a.dy = dy_dev;
    a.B = B; a.H = H; a.W = W; a.C = Cout; a.OH = p.OH; a.OW = p.OW;
    a.R = p.R; a.slab_rows = p.slab_rows; a.n_slabs = p.n_slabs;
    a.partial = (double *)workspace_dev;
    hipLaunchKernelGGL(fc_wgrad_partial, dim3((unsigned)p.n_slabs), dim3(256, 3), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fc_wgrad_final, dim3((unsigned)((27 * Cout + 255) / 256)), dim3(256), 0, s, a, dw_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
