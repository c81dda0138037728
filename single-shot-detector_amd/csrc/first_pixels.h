// What an input pixel of the first layer (Conv2d_0 / Conv1 on uint8 frames) is and where it comes from: the ONE definition
// under first_conv_ident_kernel, K1 / K1b / K1c / K1d (elementwise.hip), front_kernel / front_pool_kernel (front.hip) and
// fc_wgrad_partial (train_backbone.hip).  Device only, everything inlined: no function here becomes a call, and the weight and
// batch-norm pointers are plain pointer arguments (never through a struct), so a kernel's `const float *__restrict__`
// parameters stay scalar loads after inlining.  Every operation is separately rounded (-ffp-contract=off) except the explicit
// fmaf of the tap chain.
#pragma once
#include "ssd_internal.h"

typedef float v4f __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float act_apply(float v, int act)
{
    if (act >= 1) v = v > 0.0f ? v : 0.0f;
    if (act == 2) v = v < 6.0f ? v : 6.0f;
    return v;
}

// The pixel value p(u) = fp32(2 * fp32(u * inv255) - 1) of byte u (model.py / detector.py's normalisation in front of the first
// convolution).  A tap in the resize's zero pad band is u = 0, i.e. -1; a tap beyond the padded frame is the convolution's zero
// padding: the caller sets it to 0 AFTER this.
static __device__ __forceinline__ float fc_pixel(unsigned byte)
{
    const float inv255 = (float)(1.0 / 255.0);
    const float v = (float)byte * inv255;
    return 2.0f * v - 1.0f;
}

// The resize's index rule (resize_keeping_aspect_ratio, pipeline.py:138-194; TF r1.12 ResizeNearestNeighbor): source row / column
// of destination `dst` at scale = (float)in / (float)out over n source rows / columns.
static __device__ __forceinline__ int fc_src(int dst, float scale, int n)
{
    const int v = (int)floorf((float)dst * scale);
    return v < n - 1 ? v : n - 1;
}

// ---- a filter row of an unresized frame: the 3 pixels x 3 channels under it are 9 contiguous bytes at byte `ad`, anywhere
// inside a dword (0 or 2 bytes past a boundary on a frame of even width and an aligned base: which of the two depends on the row
// when W % 4 == 2): three aligned dword loads through a range-checked buffer resource (!live: the address is sent out of range
// and the loads return 0 without touching memory) ...
// MERGE: the second and third dword at address + 4 / + 8, which the compiler merges into ONE buffer_load_dwordx3 per row (K1b, the
// identity kernel, the weight gradient: 2-4 % of their time); else at instruction offsets 4 / 8 of three separate loads -- the
// fused kernels keep a tile's nine words in flight across a whole phase, and nine independent registers are what front_kernel's
// 244 VGPRs without scratch were reached with.
template <bool MERGE>
static __device__ __forceinline__ void fc_row_fetch(const __amdgpu_buffer_rsrc_t irsrc, bool live, int ad, unsigned &w0, unsigned &w1, unsigned &w2)
{
    const int a0 = live ? (ad & ~3) : (int)0x80000000u;
    w0 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0, 0, 0);
    w1 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, MERGE ? a0 + 4 : a0, MERGE ? 0 : 4, 0);
    w2 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, MERGE ? a0 + 8 : a0, MERGE ? 0 : 8, 0);
}

// ... and a byte alignment by sh = ad & 3: the row's bytes 0..3, 4..7, 8.. as three words
static __device__ __forceinline__ void fc_row_words(unsigned w0, unsigned w1, unsigned w2, int sh, unsigned (&d)[3])
{
    d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
    d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
    d[2] = w2 >> (8 * sh);
}

// ... nine bytes out
static __device__ __forceinline__ void fc_row_bytes(unsigned w0, unsigned w1, unsigned w2, int sh, unsigned char (&px)[9])
{
    unsigned d[3];
    fc_row_words(w0, w1, w2, sh, d);
#pragma unroll
    for (int k = 0; k < 9; ++k) px[k] = (unsigned char)(d[k >> 2] >> (8 * (k & 3)));
}

// ---- the 27 inputs of first-convolution output (cy, cx) of frame b of [B,H,W,3] frames of the network's own size, in two steps
// so that a kernel can keep a tile's bytes in flight: fetch (byte address of filter row ky: ((b H + 2 cy + ky) W + 2 cx) 3; a row
// below the frame -- row 2 cy + 2 alone, H is even -- is fetched from row 0) ...
// ROW2: only filter row 2 is tested (K1b's form); else every row, which the compiler cannot fold: the form the fused kernels and the
// identity kernel were compiled with.  The address is the same either way.
template <bool ROW2>
static __device__ __forceinline__ int frame_row_ad(int b, int H, int W, int cy, int cx, int ky)
{
    const int iy = 2 * cy + ky;
    return ((b * H + (((ROW2 && ky < 2) || iy < H) ? iy : 0)) * W + 2 * cx) * 3;
}

static __device__ __forceinline__ void frame_fetch(const __amdgpu_buffer_rsrc_t irsrc, bool live, int b, int H, int W, int cy, int cx,
                                                   unsigned (&raw)[9])
{
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
        fc_row_fetch<false>(irsrc, live, frame_row_ad<false>(b, H, W, cy, cx, ky), raw[ky * 3], raw[ky * 3 + 1], raw[ky * 3 + 2]);
}

// ... and unpack: the pixel values in (ky, kx, ci) order.  Only the taps of row 2 cy + 2 and of column 2 cx + 2 can fall outside
// the frame ('SAME' on even sizes pads bottom / right only): they are 0.
template <bool ROW2>
static __device__ __forceinline__ void frame_unpack_row(unsigned w0, unsigned w1, unsigned w2, int b, int H, int W, int cy, int cx, int ky, float (&x)[27])
{
    const bool xok = 2 * cx + 2 < W, yok = 2 * cy + 2 < H;
    unsigned char px[9];
    fc_row_bytes(w0, w1, w2, frame_row_ad<ROW2>(b, H, W, cy, cx, ky) & 3, px);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float v = fc_pixel(px[k]);
        if (ky == 2 && !yok) v = 0.0f;
        if (k >= 6 && !xok) v = 0.0f;
        x[ky * 9 + k] = v;
    }
}

static __device__ __forceinline__ void frame_unpack(const unsigned (&raw)[9], int b, int H, int W, int cy, int cx, float (&x)[27])
{
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) frame_unpack_row<false>(raw[ky * 3], raw[ky * 3 + 1], raw[ky * 3 + 2], b, H, W, cy, cx, ky, x);
}

// ... or both row by row, for a kernel that uses the bytes at once (K1b)
static __device__ __forceinline__ void frame_gather(const __amdgpu_buffer_rsrc_t irsrc, int b, int H, int W, int cy, int cx, float (&x)[27])
{
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        unsigned w0, w1, w2;
        fc_row_fetch<true>(irsrc, true, frame_row_ad<true>(b, H, W, cy, cx, ky), w0, w1, w2);
        frame_unpack_row<true>(w0, w1, w2, b, H, W, cy, cx, ky, x);
    }
}

// ---- frame b of a batch of equally sized frames whose frame 0 is g1
static __device__ __forceinline__ FrameGeom fc_frame_of(const FrameGeom &g1, int b)
{
    FrameGeom g = g1;
    g.off = g1.off + (unsigned)b * ((unsigned)g1.srcH * (unsigned)g1.srcW * 3u);
    return g;
}

// ---- the same for a RESIZED frame (geometry g; g.off: its first byte in the buffer) whose width is not reduced (g.srcW <= g.nw,
// i.e. every COCO image at min_dimension 640): the three taps of a filter row then read source columns sx(2 cx), sx(2 cx + 1),
// sx(2 cx + 2) that lie at most two pixels apart, so a filter row is still 9 contiguous source bytes from the first tap's pixel
// -- fc_row_fetch, like the frame of the network's own size -- and tap kx takes the pixel sx(2 cx + kx) - sx(2 cx) in {0, 1, 2}
// of them.  Rows are three independent source rows (any vertical scale).
static __device__ __forceinline__ int frame_row_ad_gen(const FrameGeom &g, int cy, int sx0, int ky)
{
    return (int)(g.off + (unsigned)(fc_src(2 * cy + ky, g.hs, g.srcH) * g.srcW + sx0) * 3u);
}

static __device__ __forceinline__ void frame_fetch_gen(const __amdgpu_buffer_rsrc_t irsrc, bool live, const FrameGeom &g, int cy, int cx,
                                                       unsigned (&raw)[9])
{
    const int sx0 = fc_src(2 * cx, g.ws, g.srcW);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) fc_row_fetch<false>(irsrc, live, frame_row_ad_gen(g, cy, sx0, ky), raw[ky * 3], raw[ky * 3 + 1], raw[ky * 3 + 2]);
}

static __device__ __forceinline__ void frame_unpack_gen(const unsigned (&raw)[9], int H, int W, const FrameGeom &g, int cy, int cx, float (&x)[27])
{
    const int sx0 = fc_src(2 * cx, g.ws, g.srcW);
    int off[3];
    bool xin[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        off[kx] = 3 * (fc_src(2 * cx + kx, g.ws, g.srcW) - sx0);      // 0, 3 or 6
        xin[kx] = 2 * cx + kx < g.nw;
    }
    const bool xok = 2 * cx + 2 < W;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * cy + ky;
        const bool yok = ky < 2 || iy < H;
        const bool yin = iy < g.nh;
        unsigned d[3];
        fc_row_words(raw[ky * 3], raw[ky * 3 + 1], raw[ky * 3 + 2], frame_row_ad_gen(g, cy, sx0, ky) & 3, d);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const unsigned lo = off[kx] < 4 ? d[0] : d[1], hi = off[kx] < 4 ? d[1] : d[2];
            const unsigned px = __builtin_amdgcn_alignbyte(hi, lo, off[kx] & 3);
            const bool inimg = yin && xin[kx];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float v = fc_pixel(inimg ? (px >> (8 * ci)) & 0xffu : 0u);
                if (!yok || (kx == 2 && !xok)) v = 0.0f;
                x[ky * 9 + kx * 3 + ci] = v;
            }
        }
    }
}

// ---- ... and for a resized frame of ANY geometry (the width may shrink: K1d): three source rows and three source columns per
// output, each of the nine source pixels as two aligned dwords + a byte alignment (a pixel's 3 bytes start at any byte)
static __device__ __forceinline__ void frame_gather_any(const __amdgpu_buffer_rsrc_t irsrc, const FrameGeom &g, int H, int W, int oy, int ox, float (&x)[27])
{
    int roff[3], coff[3];
    bool yin[3], xin[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int iy = 2 * oy + k, ix = 2 * ox + k;
        yin[k] = iy < g.nh;                          // else: the resize's zero pad band (or beyond the padded frame)
        xin[k] = ix < g.nw;
        roff[k] = (yin[k] ? fc_src(iy, g.hs, g.srcH) : 0) * g.srcW;
        coff[k] = xin[k] ? fc_src(ix, g.ws, g.srcW) : 0;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const bool yok = ky < 2 || 2 * oy + 2 < H;  // else: the convolution's zero padding ('SAME' on even sizes pads bottom / right only)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const bool xok = kx < 2 || 2 * ox + 2 < W;
            const unsigned p = g.off + (unsigned)(roff[ky] + coff[kx]) * 3u;
            const int a0 = (int)(p & ~3u), sh = (int)(p & 3u);
            const unsigned w0 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0, 0, 0);
            const unsigned w1 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a0, 4, 0);
            const unsigned d = __builtin_amdgcn_alignbyte(w1, w0, sh);
            const bool inimg = yin[ky] && xin[kx];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float v = fc_pixel(inimg ? (d >> (8 * ci)) & 0xffu : 0u);
                if (!(yok && xok)) v = 0.0f;
                x[(ky * 3 + kx) * 3 + ci] = v;
            }
        }
    }
}

// ---- output channels 0 .. N - 1 of one output from its 27 inputs: the (ky,kx,ci)-ordered fmaf chain over weights
// [27][row_stride] (wave-uniform: scalar loads, an SGPR operand of the fmaf), batch norm in three separately rounded steps,
// activation.  For the kernels that hold all channels of a position at once (front.hip); K1b / K1d, which walk the channels
// in chunks, keep this text in their own body (elementwise.hip first_conv_lane_body says why).  The batch norm is always there: the
// lane body's `if (mean)` (the training forward passes none) is the one difference, and a null test here made both fused kernels
// spill -- do not merge the two without their register counts in hand.
template <int N>
static __device__ __forceinline__ void fc_taps(const float (&x)[27], const float *w, int row_stride, const float *mean, const float *sf,
                                               const float *beta, int act, float (&acc)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int t = 0; t < 27; ++t) {
        const float *wr = w + t * row_stride;
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = fmaf(x[t], wr[i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float tq = (acc[i] - mean[i]) * sf[i];
        acc[i] = act_apply(tq + beta[i], act);
    }
}
