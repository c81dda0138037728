// The TRAIN head and the TRAIN FPN (include/ssd_hip.h, "the TRAIN head", "the TRAIN FPN"): forward and backward of the box
// predictor's 3x3 stride-1 'same' convolutions over a list of pyramid levels, of the FPN's 1x1, 3x3 and 3x3 stride-2 convolutions
// (one planner, one set of launches), the training-mode batch norm + ReLU that follows them, and the top-down merge's backward.
//   forward / data gradient  the exact-fp32 implicit-GEMM kernel of the inference path (igemm.hip) on a kernel that is
//                            packed ON THE DEVICE (pack_w_kernel: weights.hip's pack_conv layout, two index maps)
//   weight gradient          wgrad.hip
//   dbias, batch norm        the column statistics below: per-slab double sums, a fixed-order second stage
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`; scratch is the caller's workspace.
#include "host.h"
#include "train_head.h"

#include <algorithm>
#include <cstring>

// ----------------------------------------------------------------------------- kernel packing on the device
// w HWIO [k,k,Cin,Cout] (device), taps = k * k = 1 or 9 -> wt [taps][rows][kp] in physical channel order, zero where a channel is padding.
//   transpose == 0  the forward's kernel: row = output channel co, k = input channel ci, tap as stored
//   transpose == 1  the data gradient's kernel w'[kh,kw,co,ci] = w[2-kh,2-kw,ci,co]: row = ci, k = co, tap taps - 1 - tap (taps = 1, the
//                   1x1 data gradient: w'[0,0,co,ci] = w[0,0,ci,co])
__global__ __launch_bounds__(256) void pack_w_kernel(const float *w, int Cin, int Cout, int kp, int rows, int taps, int transpose, float *wt)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)taps * rows * kp) return;
    const int p = (int)(idx % kp), n = (int)((idx / kp) % rows), tap = (int)(idx / ((long long)kp * rows));
    const int lk = ssd_logical_of_phys(p), ln = ssd_logical_of_phys(n);
    float v = 0.0f;
    if (!transpose) {
        if (lk < Cin && ln < Cout) v = w[((long long)tap * Cin + lk) * Cout + ln];
    } else {
        if (lk < Cout && ln < Cin) v = w[((long long)(taps - 1 - tap) * Cin + ln) * Cout + lk];
    }
    wt[idx] = v;
}

// ----------------------------------------------------------------------------- column statistics
// The column-sum core of train_head.h over a level list: G = ceil(min(C, 1024) / 4) quads; a tensor wider than 1024 channels -- dbias
// only -- takes one block per 1024 channels and slab.  The second stage (stat_final; dbias: launch_slab_sum) adds a level's slabs in
// ascending order.  Both orders are fixed by the shapes alone.
static __device__ inline int th_level(const StatArgs &a, int slab)
{
    int l = 0;
    while (l + 1 < a.nlevels && slab >= a.lv[l + 1].slab_begin) ++l;
    return l;
}

// the activation's gate on the recomputed y: open where y > 0 (ReLU) and, for ReLU6, y < 6; a NaN closes it.  SSD_ACT_NONE (the
// TRAIN ShuffleNet's batch norm): there is no activation and the gate is open everywhere
static __device__ inline bool th_gate(float y, int act) { return act == SSD_ACT_NONE || (y > 0.0f && (act != SSD_ACT_RELU6 || y < 6.0f)); }

// MODE 0: sum x | 1: sum (x - mean)^2, the difference and the square in double | 2: sum g and sum g * xhat (batch-norm backward)
template <int MODE>
__global__ __launch_bounds__(256) void stat_partial(const StatArgs a)
{
    __shared__ double sm[MODE == 2 ? 2 : 1][1024];
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const int C = a.C, G = (a.CW + 3) >> 2;
    const SlabLane ln = slab_lane(tid, G, slab - L.slab_begin, a.slab_rows, L.p.rows);
    const int c0 = blockIdx.y * TH_STAT_COLS, c = c0 + ln.c;               // (blockIdx.y > 0: dbias of a layer wider than one block)
    const int vec = th_width(C);
    double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (ln.on) {
        v4f mean = {0, 0, 0, 0}, invstd = mean, gamma = mean, beta = mean;
        if (MODE >= 1) mean = th_load4(L.p.mean, c, C, vec);
        if (MODE == 2) { invstd = th_load4(L.p.invstd, c, C, vec); gamma = th_load4(L.p.gamma, c, C, vec); beta = th_load4(L.p.beta, c, C, vec); }
        for (long long r = ln.r0 + ln.rl; r < ln.r1; r += ln.rpp) {
            const v4f x = th_load4(L.p.x + r * C, c, C, vec);
            if (MODE == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0][e] += (double)x[e];
            } else if (MODE == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double d = (double)x[e] - (double)mean[e]; acc[0][e] += d * d; }
            } else {
                const v4f dy = th_load4(L.p.dy + r * C, c, C, vec);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = x[e] - mean[e], xh = t * invstd[e], sf = gamma[e] * invstd[e];
                    const float y = t * sf + beta[e];
                    const float gg = th_gate(y, a.act) ? dy[e] : 0.0f;
                    acc[0][e] += (double)gg;
                    acc[1][e] += (double)gg * (double)xh;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < (MODE == 2 ? 2 : 1); ++q) slab_reduce4(sm[q], acc[q], tid, G, a.partial + ((long long)slab * 2 + q) * C, c0, C);
}

// MODE 0: mean | 1: var, invstd, moving statistics | 2: dgamma, dbeta
template <int MODE>
__global__ __launch_bounds__(256) void stat_final(const StatArgs a)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const StatLevel &L = a.lv[blockIdx.y];
    double s = 0.0, t = 0.0;
    for (int k = L.slab_begin; k < L.slab_begin + L.n_slabs; ++k) {
        s += a.partial[((long long)k * 2) * a.C + c];
        if (MODE == 2) t += a.partial[((long long)k * 2 + 1) * a.C + c];
    }
    if (MODE == 0) L.p.mean[c] = (float)(s / (double)L.p.rows);
    if (MODE == 1) {
        const float var = (float)(s / (double)L.p.rows);
        if (L.p.var) L.p.var[c] = var;
        L.p.invstd[c] = __fdiv_rn(1.0f, sqrtf(var + a.eps));
        if (L.p.moving_mean) {
            const float mm = L.p.moving_mean[c], mv = L.p.moving_variance[c];
            L.p.moving_mean[c] = mm - (mm - L.p.mean[c]) * a.one_minus_momentum;
            L.p.moving_variance[c] = mv - (mv - var * L.unbias) * a.one_minus_momentum;
        }
    }
    if (MODE == 2) { L.p.dbeta[c] = (float)s; L.p.dgamma[c] = (float)t; }
}

// the second stage where it only sums (train_head.h): dbias over every slab of every level, the weight gradients of train_backbone.hip
__global__ __launch_bounds__(256) void slab_sum_kernel(const double *__restrict__ partial, int n_slabs, long long stride, int n,
                                                       float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < n_slabs; ++k) s += partial[k * stride + i];
    out[i] = (float)s;
}

hipError_t launch_slab_sum(const double *partial, int n_slabs, long long stride, int n, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, partial, n_slabs, stride, n, out);
    return hipGetLastError();
}

// y = act((x - mean) * sf + beta), act = ReLU, ReLU6 (elementwise.hip act_apply) or none: training -- the batch's mean, sf = gamma * invstd; inference -- the moving mean,
// sf = gamma * (1 / sqrt(moving_variance + eps)) as ssd_finalize forms it
__global__ __launch_bounds__(256) void bn_apply_forward(const StatArgs a)
{
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const SlabLane ln = slab_lane(tid, (a.CW + 3) >> 2, slab - L.slab_begin, a.slab_rows, L.p.rows);
    const int C = a.C, c = ln.c;
    if (!ln.on) return;
    const int vec = th_width(C);
    const v4f gamma = th_load4(L.p.gamma, c, C, vec), beta = th_load4(L.p.beta, c, C, vec);
    v4f mean, sf;
    if (a.training) {
        mean = th_load4(L.p.mean, c, C, vec);
        const v4f is = th_load4(L.p.invstd, c, C, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) sf[e] = gamma[e] * is[e];
    } else {
        mean = th_load4(L.p.moving_mean, c, C, vec);
        const v4f mv = th_load4(L.p.moving_variance, c, C, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) sf[e] = gamma[e] * __fdiv_rn(1.0f, sqrtf(mv[e] + a.eps));
    }
    for (long long r = ln.r0 + ln.rl; r < ln.r1; r += ln.rpp) {
        v4f x = th_load4(L.p.x + r * C, c, C, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = (x[e] - mean[e]) * sf[e];
            const float y = t + beta[e];
            float v = y > 0.0f ? y : 0.0f;
            if (a.act == SSD_ACT_RELU6) v = v < 6.0f ? v : 6.0f;
            x[e] = a.act == SSD_ACT_NONE ? y : v;
        }
        th_store4(L.p.out + r * C, c, C, vec, x);
    }
}

// dx = (gamma * invstd) * ((g - dbeta / R) - xhat * (dgamma / R)), g = dy where the gate of the recomputed y is open
__global__ __launch_bounds__(256) void bn_apply_backward(const StatArgs a)
{
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const SlabLane ln = slab_lane(tid, (a.CW + 3) >> 2, slab - L.slab_begin, a.slab_rows, L.p.rows);
    const int C = a.C, c = ln.c;
    if (!ln.on) return;
    const int vec = th_width(C);
    const v4f gamma = th_load4(L.p.gamma, c, C, vec), beta = th_load4(L.p.beta, c, C, vec), mean = th_load4(L.p.mean, c, C, vec);
    const v4f invstd = th_load4(L.p.invstd, c, C, vec), dgamma = th_load4(L.p.dgamma, c, C, vec), dbeta = th_load4(L.p.dbeta, c, C, vec);
    const float Rf = (float)L.p.rows;
    v4f sf, c1, c2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sf[e] = gamma[e] * invstd[e]; c1[e] = __fdiv_rn(dbeta[e], Rf); c2[e] = __fdiv_rn(dgamma[e], Rf); }
    for (long long r = ln.r0 + ln.rl; r < ln.r1; r += ln.rpp) {
        const v4f x = th_load4(L.p.x + r * C, c, C, vec), dy = th_load4(L.p.dy + r * C, c, C, vec);
        v4f d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = x[e] - mean[e], xh = t * invstd[e];
            const float y = t * sf[e] + beta[e];
            const float gg = th_gate(y, a.act) ? dy[e] : 0.0f;
            const float u = gg - c1[e], v = xh * c2[e];
            d[e] = sf[e] * (u - v);
        }
        th_store4(L.p.out + r * C, c, C, vec, d);
    }
}

// slabs of a level list: the slab rule on the rows of every level together, each level its own run of slabs
static void make_slabs(StatArgs &a)
{
    a.CW = a.C < TH_STAT_COLS ? a.C : TH_STAT_COLS;
    long long tot = 0;
    for (int l = 0; l < a.nlevels; ++l) tot += a.lv[l].p.rows;
    a.slab_rows = slab_rule(tot, (a.CW + 3) / 4).slab_rows;
    a.n_slabs = 0;
    for (int l = 0; l < a.nlevels; ++l) {
        a.lv[l].slab_begin = a.n_slabs;
        a.lv[l].n_slabs = (int)((a.lv[l].p.rows + a.slab_rows - 1) / a.slab_rows);
        a.n_slabs += a.lv[l].n_slabs;
    }
}

// ----------------------------------------------------------------------------- the convolutions
// One planner for the TRAIN head's 3x3 stride-1 calls and the TRAIN FPN's k x k / stride-2 / upsample-add calls: a level's
// input is [B,H,W,Cin] (Rin rows), its output [B,OH,OW,Cout] (Rout rows; stride 1: the same size).
struct ConvTrainPlan {
    int k, stride, pad, OH[TH_MAX_LEVELS], OW[TH_MAX_LEVELS];
    long long Rin[TH_MAX_LEVELS], Rout[TH_MAX_LEVELS], rin_off[TH_MAX_LEVELS], rout_off[TH_MAX_LEVELS], up_off[TH_MAX_LEVELS];
    long long Rin_tot, Rout_tot, Rup_tot;
    ConvW f, d;                         // geometry of the forward's and the data gradient's packed kernels (no pointers yet)
    int rows_per_slice, n_slices, slice_begin[TH_MAX_LEVELS], tiles_ci;
    StatArgs st;                        // dbias: the slabs of dy
    size_t off_a, off_b, off_w, off_bias, off_part, off_stat, off_up, bytes;
};

static const char *conv_plan(const ssd_conv_level *lv, int n, int B, int Cin, int Cout, int k, int stride, int with_up, ConvTrainPlan &p, bool pw_dx = false,
                             bool even_cin = false)
{
    if (!lv) return "null level list";
    if (n < 1 || n > TH_MAX_LEVELS) return "1 .. 8 levels";
    if (B < 1 || Cin < 1 || Cout < 1) return "sizes must be positive";
    if (k != 1 && k != 3) return "k must be 1 or 3";
    if (stride != 1 && stride != 2) return "stride must be 1 or 2";
    if (stride == 2 && k != 3) return "stride 2 only with k = 3";
    if (with_up && stride != 1) return "the upsample-add only with stride 1";
    if (k == 3 && Cin % 8) return "Cin must be a multiple of 8";
    if (even_cin ? (Cin % 2 || k != 1) : Cin % 4) return even_cin ? "Cin must be even (k = 1)" : "Cin must be a multiple of 4";
    if (Cin > 4096 || Cout > 4096) return "at most 4096 channels";
    const int taps = k * k;
    p.k = k; p.stride = stride; p.pad = k == 3 ? 1 : 0;
    conv_geometry(nullptr, taps, round_up(Cin, 32), round_up(Cout, 8), Cin, Cout, p.f);
    const int taps_d = k == 3 ? 9 : 1;                                  // k = 1: only ssd_pointwise_train_backward (pw_dx) runs a data gradient
    conv_geometry(nullptr, taps_d, round_up(Cout, 32), round_up(Cin, 8), Cout, Cin, p.d);
    const int widest = std::max(std::max(p.f.CinP, p.f.CoutP), std::max(p.d.CinP, p.d.CoutP));
    p.Rin_tot = p.Rout_tot = p.Rup_tot = 0;
    for (int l = 0; l < n; ++l) {
        if (lv[l].H < 1 || lv[l].W < 1) return "sizes must be positive";
        if (with_up && ((lv[l].H | lv[l].W) & 1)) return "the upsample-add needs even H and W";
        const long long R = (long long)B * lv[l].H * lv[l].W;
        if (lv[l].H > 32768 || lv[l].W > 32768 || R * widest * 4 >= (1LL << 31)) return "every level's tensors must stay below 2 GiB";
        p.OH[l] = (lv[l].H + stride - 1) / stride;
        p.OW[l] = (lv[l].W + stride - 1) / stride;
        p.Rin[l] = R;
        p.Rout[l] = (long long)B * p.OH[l] * p.OW[l];
        p.rin_off[l] = p.Rin_tot;
        p.rout_off[l] = p.Rout_tot;
        p.up_off[l] = p.Rup_tot;
        p.Rin_tot += R;
        p.Rout_tot += p.Rout[l];
        if (with_up) p.Rup_tot += R / 4;
    }
    if (p.Rin_tot >= (1LL << 31)) return "fewer than 2^31 positions in all";
    // K-slices of the weight gradient: about 1536 blocks in all
    p.tiles_ci = (Cin + 127) / 128;
    const int BN = wgrad_tile_n(Cout);
    const long long tiles = (long long)taps * p.tiles_ci * ((Cout + BN - 1) / BN);
    const long long want = std::max(1LL, 1536 / tiles);
    long long rps = (p.Rout_tot + want - 1) / want;
    if (rps < 256) rps = 256;
    rps = (rps + 15) / 16 * 16;
    p.rows_per_slice = (int)rps;
    p.n_slices = 0;
    for (int l = 0; l < n; ++l) {
        p.slice_begin[l] = p.n_slices;
        p.n_slices += (int)((p.Rout[l] + rps - 1) / rps);
    }
    memset(&p.st, 0, sizeof(p.st));
    p.st.nlevels = n;
    p.st.C = Cout;
    for (int l = 0; l < n; ++l) p.st.lv[l].p.rows = p.Rout[l];
    make_slabs(p.st);
    // workspace: [a | b | w | bias] of the forward or the data gradient (k = 3: its input is dy, or the zero-dilated dy of a
    // stride-2 layer, at the INPUT's size), then the weight gradient's partial tiles, dbias's sums and the permuted `up` tensors
    const size_t a_f = (size_t)p.Rin_tot * p.f.CinP, b_f = (size_t)p.Rout_tot * p.f.CoutP, w_f = (size_t)taps * p.f.CoutPad * p.f.CinP;
    const size_t dg = k == 3 || pw_dx ? 1 : 0;
    const size_t a_d = dg * p.Rin_tot * p.d.CinP, b_d = dg * p.Rin_tot * p.d.CoutP, w_d = dg * taps_d * p.d.CoutPad * p.d.CinP;
    p.off_a = 0;
    p.off_b = al256(std::max(a_f, a_d) * 4 + 256);
    p.off_w = p.off_b + al256(std::max(b_f, b_d) * 4 + 256);
    p.off_bias = p.off_w + al256(std::max(w_f, w_d) * 4 + 256);
    p.off_part = p.off_bias + al256((size_t)p.f.CoutP * 4 + 256);
    p.off_stat = p.off_part + al256((size_t)p.n_slices * taps * Cin * Cout * 4);
    p.off_up = p.off_stat + al256((size_t)p.st.n_slabs * 2 * Cout * 8);
    p.bytes = p.off_up + (with_up ? al256((size_t)p.Rup_tot * p.f.CoutP * 4 + 256) : 0);
    return nullptr;
}

// dy [B,OH,OW,C] logical -> D [B,H,W,Cp] physical, D[b,2oy,2ox,:] = dy[b,oy,ox,:] and zero elsewhere (and in the padding
// channels): the permute of the data gradient's operand, scattering the gradient of a stride-2 layer over the input's grid
__global__ __launch_bounds__(256) void dilate_permute_kernel(const float *__restrict__ dy, int H, int W, int OH, int OW, int C, int Cp,
                                                              long long total, float *__restrict__ out)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % Cp);
        const long long pos = idx / Cp;
        const int x = (int)(pos % W);
        const long long t = pos / W;
        const int y = (int)(t % H);
        const long long b = t / H;
        const int l = ssd_logical_of_phys(j);
        float v = 0.0f;
        if (!((x | y) & 1) && l < C) v = dy[((b * OH + (y >> 1)) * OW + (x >> 1)) * C + l];
        out[idx] = v;
    }
}

// levels of one implicit-GEMM launch: rows of `in` from in_rows[l] on, rows of `out` from out_rows[l] on
static int run_igemm(const ConvW &cw, const float *in, float *out, const float *res, const ssd_conv_level *lv, int n, int B, int stride, int pad,
                     const int *OH, const int *OW, const long long *in_rows, const long long *out_rows, const long long *res_rows, hipStream_t s)
{
    std::vector<LevelDesc> ld;
    for (int l = 0; l < n; ++l)
        ld.push_back(dense_level(lv[l].H, lv[l].W, OH ? OH[l] : lv[l].H, OW ? OW[l] : lv[l].W, cw.CoutP, in_rows[l] * cw.CinP, out_rows[l] * cw.CoutP, 0,
                                 res ? res_rows[l] * cw.CoutP : 0));
    ConvIO io{in, out};
    io.res = res;
    Op op = make_conv_op(nullptr, cw, io, B, stride, pad, SSD_ACT_NONE, ld, true);
    HIPCHK(op.run(s));
    return SSD_OK;
}

size_t conv_train_workspace(const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride, bool pw_dx, bool even_cin)
{
    ConvTrainPlan p;
    return conv_plan(levels, n_levels, B, Cin, Cout, k, stride, 0, p, pw_dx, even_cin) ? 0 : p.bytes;
}

int conv_train_forward(const std::string &fn, const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride,
                       const float *w_dev, const float *bias_dev, const float *const *up_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream, bool even_cin)
{
    ConvTrainPlan p;
    // (even_cin: the TRAIN ShuffleNet's family has ONE workspace size for both calls, the backward's with its data gradient)
    if (const char *why = conv_plan(levels, n_levels, B, Cin, Cout, k, stride, up_dev != nullptr, p, even_cin, even_cin))
        return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (!w_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, fn + ": null pointer");
    if (mis16(w_dev) || mis16(workspace_dev) || ((uintptr_t)bias_dev & 3))
        return ssd_fail(SSD_ERR_INVALID, fn + ": w_dev and workspace_dev need 16-byte alignment, bias_dev 4-byte");
    if (bias_dev && up_dev) return ssd_fail(SSD_ERR_INVALID, fn + ": bias and upsample-add are mutually exclusive");
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l].x || !levels[l].out) return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x or out is null");
        if (mis16(levels[l].x) || mis16(levels[l].out)) return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x or out is not 16-byte aligned");
        if (up_dev && (!up_dev[l] || mis16(up_dev[l]))) return ssd_fail(SSD_ERR_INVALID, fn + ": a level's up is null or not 16-byte aligned");
    }
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    float *xin = (float *)(ws + p.off_a), *outp = (float *)(ws + p.off_b), *wt = (float *)(ws + p.off_w), *biasp = (float *)(ws + p.off_bias);
    float *upp = up_dev ? (float *)(ws + p.off_up) : nullptr;
    ConvW cw = p.f;
    for (int l = 0; l < n_levels; ++l) {
        HIPCHK(launch_permute_channels(levels[l].x, p.Rin[l], Cin, cw.CinP, 1, xin + p.rin_off[l] * cw.CinP, s));
        if (up_dev) HIPCHK(launch_permute_channels(up_dev[l], p.Rin[l] / 4, Cout, cw.CoutP, 1, upp + p.up_off[l] * cw.CoutP, s));
    }
    const long long nw = (long long)cw.taps * cw.CoutPad * cw.CinP;
    LAUNCH(pack_w_kernel, dim3((unsigned)((nw + 255) / 256)), s, w_dev, Cin, Cout, cw.CinP, cw.CoutPad, cw.taps, 0, wt);
    cw.wt = wt;
    if (bias_dev) {
        HIPCHK(launch_permute_channels(bias_dev, 1, Cout, cw.CoutP, 1, biasp, s));
        cw.bias = biasp;
    }
    SSDCHK(run_igemm(cw, xin, outp, upp, levels, n_levels, B, stride, p.pad, p.OH, p.OW, p.rin_off, p.rout_off, p.up_off, s));
    for (int l = 0; l < n_levels; ++l)
        HIPCHK(launch_permute_channels(outp + p.rout_off[l] * cw.CoutP, p.Rout[l], Cout, cw.CoutP, 0, levels[l].out, s));
    return SSD_OK;
}

int conv_train_backward(const std::string &fn, const ssd_conv_level *levels, int n_levels, int B, int Cin, int Cout, int k, int stride,
                        const float *w_dev, float *dw_dev, float *dbias_dev, void *workspace_dev, size_t workspace_bytes, void *stream,
                        bool pw_dx, bool even_cin)
{
    ConvTrainPlan p;
    if (const char *why = conv_plan(levels, n_levels, B, Cin, Cout, k, stride, 0, p, pw_dx, even_cin))
        return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (!w_dev || !dw_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, fn + ": null pointer");
    if (mis16(w_dev) || mis16(dw_dev) || mis16(workspace_dev) || ((uintptr_t)dbias_dev & 3))
        return ssd_fail(SSD_ERR_INVALID, fn + ": w_dev, dw_dev and workspace_dev need 16-byte alignment, dbias_dev 4-byte");
    int with_dx = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l].x || !levels[l].dy) return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x or dy is null");
        if (mis16(levels[l].x) || mis16(levels[l].dy) || mis16(levels[l].out))
            return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x, dy or out is not 16-byte aligned");
        with_dx += levels[l].out ? 1 : 0;
    }
    if (with_dx != 0 && with_dx != n_levels)
        return ssd_fail(SSD_ERR_INVALID, fn + ": dx (out) must be given for every level or for none");
    if (with_dx && k == 1 && !pw_dx) return ssd_fail(SSD_ERR_INVALID, fn + ": no data gradient of a 1x1 convolution (dx must be NULL)");
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    if (with_dx) {          // dx = conv_same(dy, w'), stride 2: of the zero-dilated dy: the forward's launch on the rotated, transposed kernel
        float *dyp = (float *)(ws + p.off_a), *dxp = (float *)(ws + p.off_b), *wt = (float *)(ws + p.off_w);
        ConvW cw = p.d;
        for (int l = 0; l < n_levels; ++l) {
            float *dst = dyp + p.rin_off[l] * cw.CinP;
            if (stride == 1) {
                HIPCHK(launch_permute_channels(levels[l].dy, p.Rin[l], Cout, cw.CinP, 1, dst, s));
            } else {
                const long long total = p.Rin[l] * cw.CinP;
                const long long blocks = std::min<long long>((total + 255) / 256, 256 * 32);
                LAUNCH(dilate_permute_kernel, dim3((unsigned)blocks), s, levels[l].dy, levels[l].H, levels[l].W, p.OH[l], p.OW[l], Cout, cw.CinP, total, dst);
            }
        }
        const long long nw = (long long)cw.taps * cw.CoutPad * cw.CinP;
        LAUNCH(pack_w_kernel, dim3((unsigned)((nw + 255) / 256)), s, w_dev, Cin, Cout, cw.CinP, cw.CoutPad, cw.taps, 1, wt);
        cw.wt = wt;
        SSDCHK(run_igemm(cw, dyp, dxp, nullptr, levels, n_levels, B, 1, p.pad, nullptr, nullptr, p.rin_off, p.rin_off, nullptr, s));
        for (int l = 0; l < n_levels; ++l)
            HIPCHK(launch_permute_channels(dxp + p.rin_off[l] * cw.CoutP, p.Rin[l], Cin, cw.CoutP, 0, levels[l].out, s));
    }
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.nlevels = n_levels; a.Cin = Cin; a.Cout = Cout;
    a.k = k; a.stride = stride; a.pad = p.pad;
    a.rows_per_slice = p.rows_per_slice; a.n_slices = p.n_slices; a.tiles_ci = p.tiles_ci;
    a.partial = (float *)(ws + p.off_part);
    for (int l = 0; l < n_levels; ++l) {
        WgradLevel &L = a.lv[l];
        L.x = levels[l].x; L.dy = levels[l].dy; L.H = levels[l].H; L.W = levels[l].W;
        L.OW = p.OW[l]; L.P = p.OH[l] * p.OW[l]; L.R = (int)p.Rout[l];
        L.slice_begin = p.slice_begin[l];
        L.dP = ssd_udiv_make((unsigned)L.P);
        L.dOW = ssd_udiv_make((unsigned)L.OW);
    }
    HIPCHK(launch_wgrad(a, dw_dev, s));
    if (dbias_dev) {
        StatArgs st = p.st;
        st.partial = (double *)(ws + p.off_stat);
        for (int l = 0; l < n_levels; ++l) st.lv[l].p.x = levels[l].dy;
        LAUNCH(stat_partial<0>, dim3((unsigned)st.n_slabs, (unsigned)((Cout + TH_STAT_COLS - 1) / TH_STAT_COLS)), s, st);
        HIPCHK(launch_slab_sum(st.partial, st.n_slabs, 2LL * Cout, Cout, dbias_dev, s));
    }
    return SSD_OK;
}

// the TRAIN head's entry points: k = 3, stride 1, no upsample-add
extern "C" size_t ssd_conv3x3_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout)
{
    ConvTrainPlan p;
    return conv_plan(levels, n_levels, B, Cin, Cout, 3, 1, 0, p) ? 0 : p.bytes;
}

extern "C" int ssd_conv3x3_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                         const float *w_dev, const float *bias_dev, void *workspace_dev, size_t workspace_bytes,
                                         void *stream)
{
    return conv_train_forward("ssd_conv3x3_train_forward", levels, n_levels, B, Cin, Cout, 3, 1, w_dev, bias_dev, nullptr, workspace_dev,
                              workspace_bytes, stream);
}

extern "C" int ssd_conv3x3_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                          const float *w_dev, float *dw_dev, float *dbias_dev, void *workspace_dev,
                                          size_t workspace_bytes, void *stream)
{
    return conv_train_backward("ssd_conv3x3_train_backward", levels, n_levels, B, Cin, Cout, 3, 1, w_dev, dw_dev, dbias_dev, workspace_dev,
                               workspace_bytes, stream);
}

// the TRAIN FPN's entry points
extern "C" size_t ssd_conv_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                                 int32_t k, int32_t stride, int32_t with_up)
{
    ConvTrainPlan p;
    return conv_plan(levels, n_levels, B, Cin, Cout, k, stride, with_up != 0, p) ? 0 : p.bytes;
}

extern "C" int ssd_conv_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout, int32_t k,
                                      int32_t stride, const float *w_dev, const float *bias_dev, const float *const *up_dev,
                                      void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return conv_train_forward("ssd_conv_train_forward", levels, n_levels, B, Cin, Cout, k, stride, w_dev, bias_dev, up_dev, workspace_dev,
                              workspace_bytes, stream);
}

extern "C" int ssd_conv_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout, int32_t k,
                                       int32_t stride, const float *w_dev, float *dw_dev, float *dbias_dev, void *workspace_dev,
                                       size_t workspace_bytes, void *stream)
{
    return conv_train_backward("ssd_conv_train_backward", levels, n_levels, B, Cin, Cout, k, stride, w_dev, dw_dev, dbias_dev, workspace_dev,
                               workspace_bytes, stream);
}

// the TRAIN backbone's 1x1 backward: ssd_conv_train_backward with k = 1 and, where the levels carry `out`, the data gradient
extern "C" size_t ssd_pointwise_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout)
{
    ConvTrainPlan p;
    return conv_plan(levels, n_levels, B, Cin, Cout, 1, 1, 0, p, true) ? 0 : p.bytes;
}

extern "C" int ssd_pointwise_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                            const float *w_dev, float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return conv_train_backward("ssd_pointwise_train_backward", levels, n_levels, B, Cin, Cout, 1, 1, w_dev, dw_dev, nullptr, workspace_dev,
                               workspace_bytes, stream, true);
}

// ----------------------------------------------------------------------------- the top-down merge's backward
// out = base + g[2y,2x] + g[2y,2x+1] + g[2y+1,2x] + g[2y+1,2x+1] (same == 0, g [B,2H,2W,C]) or out = base + g (same != 0), left
// to right; a NULL base starts at +0, and where gate > 0 is false every g term reads as +0.  One thread per channel quad.
__global__ __launch_bounds__(256) void fpn_merge_backward_kernel(const float *base, const float *__restrict__ g, const float *__restrict__ gate,
                                                                  float *out, long long rows, int H, int W, int C, int same)
{
    const int CQ = (C + 3) >> 2;
    const int vec = (C & 3) == 0 ? 4 : 1;
    const long long total = rows * CQ;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)(idx % CQ) << 2;
        const long long r = idx / CQ;
        v4f acc = {0.f, 0.f, 0.f, 0.f}, open = {1.f, 1.f, 1.f, 1.f};
        if (base) acc = th_load4(base + r * C, c, C, vec);
        if (gate) open = th_load4(gate + r * C, c, C, vec);
        if (same) {
            const v4f t = th_load4(g + r * C, c, C, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + (open[e] > 0.0f ? t[e] : 0.0f);
        } else {
            const int x = (int)(r % W);
            const long long q = r / W;
            const int y = (int)(q % H);
            const long long b = q / H;
            const long long g0 = ((b * 2 * H + 2 * y) * 2 * W + 2 * x) * C;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const v4f v = th_load4(g + g0 + ((long long)(t >> 1) * 2 * W + (t & 1)) * C, c, C, vec);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + (open[e] > 0.0f ? v[e] : 0.0f);
            }
        }
        th_store4(out + r * C, c, C, vec, acc);
    }
}

extern "C" int ssd_fpn_merge_backward(const float *base_dev, const float *g_dev, const float *gate_dev, int32_t B, int32_t H, int32_t W,
                                      int32_t C, int32_t same_size, float *out_dev, void *stream)
{
    if (!g_dev || !out_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_fpn_merge_backward: g_dev or out_dev is null");
    if (B < 1 || H < 1 || W < 1 || C < 1 || B > 65536 || H > 16384 || W > 16384 || C > 4096 || (same_size != 0 && same_size != 1))
        return ssd_fail(SSD_ERR_INVALID, "ssd_fpn_merge_backward: B, H, W, C >= 1, B <= 65536, H and W <= 16384, C <= 4096, same_size 0 or 1");
    if ((long long)B * H * W * C * (same_size ? 1 : 4) >= (1LL << 40)) return ssd_fail(SSD_ERR_INVALID, "ssd_fpn_merge_backward: tensor too large");
    if (mis16(base_dev) || mis16(g_dev) || mis16(gate_dev) || mis16(out_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_fpn_merge_backward: every pointer needs 16-byte alignment");
    if (out_dev == g_dev || (gate_dev && out_dev == gate_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_fpn_merge_backward: out_dev may alias base_dev only");
    const long long rows = (long long)B * H * W, total = rows * ((C + 3) / 4);
    const long long blocks = std::min<long long>((total + 255) / 256, 256 * 32);
    LAUNCH(fpn_merge_backward_kernel, dim3((unsigned)blocks), (hipStream_t)stream, base_dev, g_dev, gate_dev, out_dev, rows, H, W, C, same_size);
    return SSD_OK;
}

// ----------------------------------------------------------------------------- batch norm + ReLU
static const char *bn_plan(const ssd_bn_level *lv, int n, int C, StatArgs &a)
{
    if (!lv) return "null level list";
    if (n < 1 || n > TH_MAX_LEVELS) return "1 .. 8 levels";
    if (C < 1 || C > 1024) return "1 .. 1024 channels";
    memset(&a, 0, sizeof(a));
    a.nlevels = n;
    a.C = C;
    for (int l = 0; l < n; ++l) {
        if (lv[l].rows < 1 || lv[l].rows >= (1LL << 40)) return "rows must be positive";
        a.lv[l].p.rows = lv[l].rows;
    }
    make_slabs(a);
    return nullptr;
}

extern "C" size_t ssd_bn_relu_train_workspace_bytes(const ssd_bn_level *levels, int32_t n_levels, int32_t C)
{
    StatArgs a;
    return bn_plan(levels, n_levels, C, a) ? 0 : al256((size_t)a.n_slabs * 2 * C * 8);
}

static void bn_fill(StatArgs &a, const ssd_bn_level *lv)
{
    for (int l = 0; l < a.nlevels; ++l) {
        StatLevel &L = a.lv[l];
        L.p = lv[l];
        L.unbias = L.p.rows > 1 ? (float)((double)L.p.rows / (double)(L.p.rows - 1)) : 1.0f;
    }
}

int bn_train_forward(const std::string &fn, const ssd_bn_level *levels, int n_levels, int C, int act, int training, float epsilon,
                     float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream, bool none_ok)
{
    StatArgs a;
    if (const char *why = bn_plan(levels, n_levels, C, a)) return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (act != SSD_ACT_RELU && act != SSD_ACT_RELU6 && !(none_ok && act == SSD_ACT_NONE))
        return ssd_fail(SSD_ERR_INVALID, fn + (none_ok ? ": act must be SSD_ACT_NONE, SSD_ACT_RELU or SSD_ACT_RELU6" : ": act must be SSD_ACT_RELU or SSD_ACT_RELU6"));
    if (!(epsilon > 0.0f) || !(epsilon < 1e30f) || !(one_minus_momentum >= 0.0f) || !(one_minus_momentum <= 1.0f) || (training != 0 && training != 1))
        return ssd_fail(SSD_ERR_INVALID, fn + ": epsilon > 0, 0 <= one_minus_momentum <= 1, training 0 or 1");
    for (int l = 0; l < n_levels; ++l) {
        const ssd_bn_level &L = levels[l];
        if (!L.x || !L.out || !L.gamma || !L.beta) return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x, out, gamma or beta is null");
        if (training ? (!L.mean || !L.invstd) : (!L.moving_mean || !L.moving_variance))
            return ssd_fail(SSD_ERR_INVALID, fn + ": training needs mean and invstd, inference the moving statistics");
        if ((L.moving_mean == nullptr) != (L.moving_variance == nullptr))
            return ssd_fail(SSD_ERR_INVALID, fn + ": the moving statistics must be given together");
        if (mis16(L.x) || mis16(L.out) || mis16(L.gamma) || mis16(L.beta) || mis16(L.moving_mean) || mis16(L.moving_variance) || mis16(L.mean) ||
            mis16(L.var) || mis16(L.invstd))
            return ssd_fail(SSD_ERR_INVALID, fn + ": every pointer needs 16-byte alignment");
    }
    if (training && (!workspace_dev || mis16(workspace_dev))) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace_dev null or misaligned");
    if (training && workspace_bytes < al256((size_t)a.n_slabs * 2 * C * 8)) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace too small");
    bn_fill(a, levels);
    a.partial = (double *)workspace_dev;
    a.eps = epsilon; a.one_minus_momentum = one_minus_momentum; a.training = training; a.act = act;
    hipStream_t s = (hipStream_t)stream;
    const dim3 gf((unsigned)((C + 255) / 256), (unsigned)n_levels);
    if (training) {
        LAUNCH(stat_partial<0>, dim3((unsigned)a.n_slabs), s, a);
        LAUNCH(stat_final<0>, gf, s, a);
        LAUNCH(stat_partial<1>, dim3((unsigned)a.n_slabs), s, a);
        LAUNCH(stat_final<1>, gf, s, a);
    }
    LAUNCH(bn_apply_forward, dim3((unsigned)a.n_slabs), s, a);
    return SSD_OK;
}

int bn_train_backward(const std::string &fn, const ssd_bn_level *levels, int n_levels, int C, int act, void *workspace_dev,
                      size_t workspace_bytes, void *stream, bool none_ok)
{
    StatArgs a;
    if (const char *why = bn_plan(levels, n_levels, C, a)) return ssd_fail(SSD_ERR_INVALID, fn + ": " + why);
    if (act != SSD_ACT_RELU && act != SSD_ACT_RELU6 && !(none_ok && act == SSD_ACT_NONE))
        return ssd_fail(SSD_ERR_INVALID, fn + (none_ok ? ": act must be SSD_ACT_NONE, SSD_ACT_RELU or SSD_ACT_RELU6" : ": act must be SSD_ACT_RELU or SSD_ACT_RELU6"));
    for (int l = 0; l < n_levels; ++l) {
        const ssd_bn_level &L = levels[l];
        if (!L.x || !L.dy || !L.out || !L.gamma || !L.beta || !L.mean || !L.invstd || !L.dgamma || !L.dbeta)
            return ssd_fail(SSD_ERR_INVALID, fn + ": a level's x, dy, out, gamma, beta, mean, invstd, dgamma or dbeta is null");
        if (mis16(L.x) || mis16(L.dy) || mis16(L.out) || mis16(L.gamma) || mis16(L.beta) || mis16(L.mean) || mis16(L.invstd) || mis16(L.dgamma) ||
            mis16(L.dbeta))
            return ssd_fail(SSD_ERR_INVALID, fn + ": every pointer needs 16-byte alignment");
    }
    if (!workspace_dev || mis16(workspace_dev)) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace_dev null or misaligned");
    if (workspace_bytes < al256((size_t)a.n_slabs * 2 * C * 8)) return ssd_fail(SSD_ERR_INVALID, fn + ": workspace too small");
    bn_fill(a, levels);
    a.partial = (double *)workspace_dev;
    a.act = act;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(stat_partial<2>, dim3((unsigned)a.n_slabs), s, a);
    LAUNCH(stat_final<2>, dim3((unsigned)((C + 255) / 256), (unsigned)n_levels), s, a);
    LAUNCH(bn_apply_backward, dim3((unsigned)a.n_slabs), s, a);
    return SSD_OK;
}

// the TRAIN head's pair is the ReLU case of the TRAIN backbone's
extern "C" int ssd_bn_relu_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t training, float epsilon,
                                         float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return bn_train_forward("ssd_bn_relu_train_forward", levels, n_levels, C, SSD_ACT_RELU, training, epsilon, one_minus_momentum, workspace_dev,
                            workspace_bytes, stream);
}

extern "C" int ssd_bn_relu_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, void *workspace_dev,
                                          size_t workspace_bytes, void *stream)
{
    return bn_train_backward("ssd_bn_relu_train_backward", levels, n_levels, C, SSD_ACT_RELU, workspace_dev, workspace_bytes, stream);
}

extern "C" int ssd_bn_act_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, int32_t training, float epsilon,
                                        float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return bn_train_forward("ssd_bn_act_train_forward", levels, n_levels, C, act, training, epsilon, one_minus_momentum, workspace_dev,
                            workspace_bytes, stream);
}

extern "C" int ssd_bn_act_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, void *workspace_dev,
                                         size_t workspace_bytes, void *stream)
{
    return bn_train_backward("ssd_bn_act_train_backward", levels, n_levels, C, act, workspace_dev, workspace_bytes, stream);
}
