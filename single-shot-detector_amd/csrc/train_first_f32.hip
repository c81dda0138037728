// The TRAIN first convolution from float frames (include/ssd_hip.h, the header block of that name): Conv2d_0 / Conv1's raw forward
// and its weight gradient on float32 [B,H,W,3] frames, the batches TrainPipeline yields.  The siblings of first_conv_px_kernel
// (elementwise.hip) and fc_wgrad_partial (train_backbone.hip) on the float pixel source of first_pixels_f32.h: the same fmaf
// chain, the same slab order (train_head.h's column-sum core), so frames on the byte grid give the uint8 block's bits.
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`; scratch is the caller's workspace.
#include "host.h"
#include "train_head.h"
#include "first_pixels_f32.h"

#include <atomic>

// the plan of a call (fc32_plan) and, with the pointers, the weight gradient's launch arguments
struct Fc32Args {
    const float *img, *dy;
    int B, H, W, C, OH, OW;          // C = Cout
    Slabs sl;                        // of the OUTPUT rows B * OH * OW
    double *partial;                 // [n_slabs][27][C]
};

static const char *fc32_plan(int B, int H, int W, int Cout, Fc32Args &p)
{
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be positive";
    if ((H & 1) || (W & 1)) return "H and W must be even (the network's own size)";
    if (Cout < 4 || Cout > 64 || Cout % 4) return "Cout must be a multiple of 4 and at most 64";
    if ((long long)B * H * W * 12 >= (1LL << 31)) return "B * H * W * 12 bytes of frames must stay below 2^31";
    p.B = B; p.H = H; p.W = W; p.C = Cout;
    p.OH = H / 2;
    p.OW = W / 2;
    p.sl = slab_rule((long long)B * p.OH * p.OW, Cout / 4);
    return nullptr;
}

static size_t fc32_bytes(const Fc32Args &p) { return al256((size_t)p.sl.n_slabs * 27 * p.C * 8); }

static __device__ __forceinline__ __amdgpu_buffer_rsrc_t fc32_frames(const float *img, int B, int H, int W)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)img, 0, (int)((long long)B * H * W * 12), 0x00020000);
}

// ----------------------------------------------------------------------------- the forward
// first_conv_px_kernel's form without batch norm: one LANE = one output pixel, all channels.  The 27 values are fetched and
// normalised once per pixel (a tap outside the frame is 0: fmaf(0, w, acc)), the weights are wave-uniform (scalar loads, an SGPR
// operand of the fmaf), channels go in chunks of CH accumulators (8, or 4 where Cout % 8 == 4) through ONE fmaf chain per output
// from +0 in (ky,kx,ci) order, and the finished rows leave through a per-wave LDS transpose (rows padded by FC32_ROWPAD floats),
// so that a store instruction writes 1 KB of consecutive bytes: the wave's 64 pixels are 64 * Cout * 4 consecutive bytes of the
// output.  A wave = 64 consecutive outputs, a block = 256: the grid covers the batch in one pass (no stride).
#define FC32_ROWPAD 4
template <int CH>
__global__ __launch_bounds__(256) void fc32_forward_kernel(const float *__restrict__ img, int B, int H, int W, const float *__restrict__ w, int Cout,
                                                            float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float fc32_tr[];     // [4 waves][64 pixels][Cout + FC32_ROWPAD]
    const __amdgpu_buffer_rsrc_t irsrc = fc32_frames(img, B, H, W);
    const int OH = H >> 1, OW = W >> 1;
    const long long total = (long long)B * OH * OW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rowf = Cout + FC32_ROWPAD;
    float *reg = fc32_tr + (size_t)wave * 64 * rowf;
    const long long wbase = ((long long)blockIdx.x * 4 + wave) * 64;
    if (wbase >= total) return;                                          // wave-uniform; no block barrier below
    const long long pix = wbase + lane;
    const long long pp = pix < total ? pix : total - 1;
    const int ox = (int)(pp % OW);
    const int row = (int)(pp / OW);                                      // b * OH + oy: image row of tap ky is 2 * row + ky
    const int oy = row % OH;
    const bool yok = oy < OH - 1, xok = ox < OW - 1;                     // else row H / column W: outside
    float x[27];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const bool live = ky < 2 || yok;
        float r[9];
        f32_row_fetch(irsrc, live, xok, live ? f32_row_ad(2 * row + ky, W, ox) : 0, r);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            float v = r[k];
            if (!live) v = 0.0f;
            if (k >= 6 && !xok) v = 0.0f;
            x[ky * 9 + k] = v;
        }
    }
#pragma unroll 1
    for (int ch = 0; ch < Cout; ch += CH) {                              // wave-uniform (not unrolled: the weights do not fit the SGPRs)
        float acc[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            const float *wr = w + t * Cout + ch;
#pragma unroll
            for (int i = 0; i < CH; ++i) acc[i] = fmaf(x[t], wr[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < CH; i += 4) *(v4f *)(reg + lane * rowf + ch + i) = (v4f){acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
    }
    // the wave's rows -> 64 * Cout * 4 consecutive bytes of the output, 16 B per lane and instruction (wave-private LDS region:
    // the wave's own ds_writes are ordered before its ds_reads by the counter wait the compiler places)
    const int LP = Cout >> 2;                                            // 16-B pieces per pixel
    const long long nlive = (total - wbase < 64 ? total - wbase : 64) * LP;
    float *obase = out + wbase * Cout;
    for (int q = lane; q < 64 * LP; q += 64) {
        const int p = q / LP, c4 = q - p * LP;
        const v4f v = *(const v4f *)(reg + p * rowf + c4 * 4);
        if (q < nlive) *(v4f *)(obase + (long long)q * 4) = v;
    }
}

// ----------------------------------------------------------------------------- the weight gradient
// fc_wgrad_partial's sibling, the same block shape so that the order rule is literally shared: block = slab of output rows x the
// three filter rows; thread (ky = threadIdx.y, tid = threadIdx.x) is lane tid of the column-sum core, G = C / 4, for filter row
// ky and keeps the sums of q * dy of that row -- 3 pixels x 3 channels x 4 output channels, 36 doubles.  The nine values under a
// filter row come from f32_row_fetch (first_pixels_f32.h), as in the forward.  Only row 2oy+2 and column 2ox+2 can lie outside
// the image: such taps are skipped.  The product of two floats is exact in double, so fma(q, dy, acc) has the bits of
// acc + q * dy.  The block then adds its row lanes one tap at a time, each filter row in its own third of the LDS.
__global__ __launch_bounds__(768) void fc32_wgrad_partial(const Fc32Args a)
{
    __shared__ double sm[3][1024];
    const int tid = threadIdx.x, ky = threadIdx.y, slab = blockIdx.x;
    const int C = a.C, G = C >> 2;
    const SlabLane ln = slab_lane(tid, G, slab, a.sl.slab_rows, a.sl.R);
    const int c = ln.c, rpp = ln.rpp;
    const long long r0 = ln.r0, r1 = ln.r1;
    const __amdgpu_buffer_rsrc_t irsrc = fc32_frames(a.img, a.B, a.H, a.W);
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
            const bool col2 = cx < OW - 1;                   // else column W: outside
            float px[9];
            f32_row_fetch(irsrc, true, col2, f32_row_ad(2 * crow + ky, a.W, cx), px);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double pv = (double)px[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k][e] = fma(pv, dd[e], acc[k][e]);
            }
            if (col2) {
#pragma unroll
                for (int k = 6; k < 9; ++k) {
                    const double pv = (double)px[k];
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

// ----------------------------------------------------------------------------- the entry points
extern "C" int ssd_first_conv_f32_train_forward(const float *images_dev, int32_t B, int32_t H, int32_t W, const float *w_dev, int32_t Cout,
                                                float *out_dev, void *stream)
{
    Fc32Args p;
    if (const char *why = fc32_plan(B, H, W, Cout, p)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_f32_train_forward: ") + why);
    if (!images_dev || !w_dev || !out_dev)
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_f32_train_forward: null pointer (images_dev, w_dev, out_dev)");
    if (mis16(images_dev) || mis16(w_dev) || mis16(out_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_f32_train_forward: images_dev, w_dev and out_dev need 16-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    const long long px = (long long)B * p.OH * p.OW;
    const dim3 grid((unsigned)((px + 255) / 256)), blk(256);             // < 2^31 / 48 / 256 blocks
    const size_t lds = (size_t)256 * (Cout + FC32_ROWPAD) * sizeof(float);
    if (Cout % 8 == 0) {
        // 64 channels: 68 KB of transpose rows, above the 64 KB a kernel gets without asking, so ask -- per device
        static std::atomic<unsigned> attr_done{0};
        if (lds > 65536) HIPCHK(ssd_allow_lds((const void *)fc32_forward_kernel<8>, (int)lds, attr_done));
        hipLaunchKernelGGL(fc32_forward_kernel<8>, grid, blk, lds, s, images_dev, B, H, W, w_dev, Cout, out_dev);
    } else
        hipLaunchKernelGGL(fc32_forward_kernel<4>, grid, blk, lds, s, images_dev, B, H, W, w_dev, Cout, out_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

extern "C" size_t ssd_first_conv_f32_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout)
{
    Fc32Args p;
    return fc32_plan(B, H, W, Cout, p) ? 0 : fc32_bytes(p);
}

extern "C" int ssd_first_conv_f32_train_backward(const float *images_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t Cout,
                                                 float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    Fc32Args a;
    if (const char *why = fc32_plan(B, H, W, Cout, a)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_first_conv_f32_train_backward: ") + why);
    if (!images_dev || !dy_dev || !dw_dev || !workspace_dev)
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_f32_train_backward: null pointer (images_dev, dy_dev, dw_dev, workspace_dev)");
    if (mis16(images_dev) || mis16(dy_dev) || mis16(dw_dev) || mis16(workspace_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_f32_train_backward: images_dev, dy_dev, dw_dev and workspace_dev need 16-byte alignment");
    if (workspace_bytes < fc32_bytes(a)) return ssd_fail(SSD_ERR_INVALID, "ssd_first_conv_f32_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    a.img = images_dev; a.dy = dy_dev;
    a.partial = (double *)workspace_dev;
    hipLaunchKernelGGL(fc32_wgrad_partial, dim3((unsigned)a.sl.n_slabs), dim3(256, 3), 0, s, a);   // 256 x 3: not LAUNCH's block
    HIPCHK(hipGetLastError());
    HIPCHK(launch_slab_sum(a.partial, a.sl.n_slabs, 27LL * Cout, 27 * Cout, dw_dev, s));
    return SSD_OK;
}
