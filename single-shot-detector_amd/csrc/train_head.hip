// The TRAIN head (include/ssd_hip.h, "the TRAIN head"): forward and backward of the box predictor's 3x3 stride-1 'same'
// convolutions over a list of pyramid levels, and the training-mode batch norm + ReLU that follows each tower layer.
//   forward / data gradient  the exact-fp32 implicit-GEMM kernel of the inference path (igemm.hip) on a kernel that is
//                            packed ON THE DEVICE (pack_w_kernel: weights.hip's pack_conv layout, two index maps)
//   weight gradient          wgrad.hip
//   dbias, batch norm        the column statistics below: per-slab double sums, a fixed-order second stage
// Every call checks its arguments before the first HIP call, then only enqueues on `stream`; scratch is the caller's workspace.
#include "host.h"
#include "train_head.h"

#include <algorithm>
#include <cstring>

typedef float v4f __attribute__((ext_vector_type(4)));

static inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// ----------------------------------------------------------------------------- kernel packing on the device
// w HWIO [3,3,Cin,Cout] (device) -> wt [9][rows][kp] in physical channel order, zero where a channel is padding.
//   transpose == 0  the forward's kernel: row = output channel co, k = input channel ci, tap as stored
//   transpose == 1  the data gradient's kernel w'[kh,kw,co,ci] = w[2-kh,2-kw,ci,co]: row = ci, k = co, tap 8 - tap
__global__ __launch_bounds__(256) void pack_w_kernel(const float *w, int Cin, int Cout, int kp, int rows, int transpose, float *wt)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9LL * rows * kp) return;
    const int p = (int)(idx % kp), n = (int)((idx / kp) % rows), tap = (int)(idx / ((long long)kp * rows));
    const int lk = ssd_logical_of_phys(p), ln = ssd_logical_of_phys(n);
    float v = 0.0f;
    if (!transpose) {
        if (lk < Cin && ln < Cout) v = w[((long long)tap * Cin + lk) * Cout + ln];
    } else {
        if (lk < Cout && ln < Cin) v = w[((long long)(8 - tap) * Cin + ln) * Cout + lk];
    }
    wt[idx] = v;
}

// ----------------------------------------------------------------------------- column statistics
// Thread (rl = tid / G, g = tid % G) of a block walks the rows r0 + rl, r0 + rl + rpp, ... of its slab for the channel quad g
// (G = ceil(min(C, 1024) / 4) quads, rpp = 256 / G rows per pass; a tensor wider than 1024 channels -- dbias only -- takes one
// block per 1024 channels and slab), adding in double; the block then adds its rpp row lanes in ascending
// order.  The second stage (stat_final) adds a level's slabs in ascending order.  Both orders are fixed by the shapes alone.
static __device__ inline int th_level(const StatArgs &a, int slab)
{
    int l = 0;
    while (l + 1 < a.nlevels && slab >= a.lv[l + 1].slab_begin) ++l;
    return l;
}

// MODE 0: sum x | 1: sum (x - mean)^2, the difference and the square in double | 2: sum g and sum g * xhat (batch-norm backward)
template <int MODE>
__global__ __launch_bounds__(256) void stat_partial(const StatArgs a)
{
    __shared__ double sm[MODE == 2 ? 2 : 1][1024];
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const int C = a.C, G = (a.CW + 3) >> 2, rpp = 256 / G;
    const int rl = tid / G, g = tid - rl * G, c = blockIdx.y * TH_STAT_COLS + (g << 2);     // (blockIdx.y > 0: dbias of a layer wider than one block)
    const bool vec = (C & 3) == 0;
    const long long r0 = (long long)(slab - L.slab_begin) * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < L.p.rows ? r0 + a.slab_rows : L.p.rows;
    double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (rl < rpp) {
        v4f mean = {0, 0, 0, 0}, invstd = mean, gamma = mean, beta = mean;
        if (MODE >= 1) mean = th_load4(L.p.mean, c, C, vec);
        if (MODE == 2) { invstd = th_load4(L.p.invstd, c, C, vec); gamma = th_load4(L.p.gamma, c, C, vec); beta = th_load4(L.p.beta, c, C, vec); }
        for (long long r = r0 + rl; r < r1; r += rpp) {
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
                    const float gg = y > 0.0f ? dy[e] : 0.0f;
                    acc[0][e] += (double)gg;
                    acc[1][e] += (double)gg * (double)xh;
                }
            }
        }
    }
    constexpr int NQ = MODE == 2 ? 2 : 1;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) sm[q][tid * 4 + e] = acc[q][e];
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = 0.0;
                for (int j = 0; j < rpp; ++j) s += sm[q][(j * G + g) * 4 + e];
                if (c + e < C) a.partial[((long long)slab * 2 + q) * C + c + e] = s;
            }
    }
}

// MODE 0: mean | 1: var, invstd, moving statistics | 2: dgamma, dbeta | 3: the sum over every slab of every level -> lv[0].out (dbias)
template <int MODE>
__global__ __launch_bounds__(256) void stat_final(const StatArgs a)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const StatLevel &L = a.lv[blockIdx.y];
    const int s0 = MODE == 3 ? 0 : L.slab_begin, s1 = MODE == 3 ? a.n_slabs : L.slab_begin + L.n_slabs;
    double s = 0.0, t = 0.0;
    for (int k = s0; k < s1; ++k) {
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
    if (MODE == 3) L.p.out[c] = (float)s;
}

// y = relu((x - mean) * sf + beta): training -- the batch's mean, sf = gamma * invstd; inference -- the moving mean,
// sf = gamma * (1 / sqrt(moving_variance + eps)) as ssd_finalize forms it
__global__ __launch_bounds__(256) void bn_apply_forward(const StatArgs a)
{
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const int C = a.C, G = (a.CW + 3) >> 2, rpp = 256 / G;
    const int rl = tid / G, g = tid - rl * G, c = g << 2;
    if (rl >= rpp) return;
    const bool vec = (C & 3) == 0;
    const long long r0 = (long long)(slab - L.slab_begin) * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < L.p.rows ? r0 + a.slab_rows : L.p.rows;
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
    for (long long r = r0 + rl; r < r1; r += rpp) {
        v4f x = th_load4(L.p.x + r * C, c, C, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = (x[e] - mean[e]) * sf[e];
            const float y = t + beta[e];
            x[e] = y > 0.0f ? y : 0.0f;
        }
        th_store4(L.p.out + r * C, c, C, vec, x);
    }
}

// dx = (gamma * invstd) * ((g - dbeta / R) - xhat * (dgamma / R)), g = dy where the recomputed y > 0
__global__ __launch_bounds__(256) void bn_apply_backward(const StatArgs a)
{
    const int tid = threadIdx.x, slab = blockIdx.x;
    const StatLevel &L = a.lv[th_level(a, slab)];
    const int C = a.C, G = (a.CW + 3) >> 2, rpp = 256 / G;
    const int rl = tid / G, g = tid - rl * G, c = g << 2;
    if (rl >= rpp) return;
    const bool vec = (C & 3) == 0;
    const long long r0 = (long long)(slab - L.slab_begin) * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < L.p.rows ? r0 + a.slab_rows : L.p.rows;
    const v4f gamma = th_load4(L.p.gamma, c, C, vec), beta = th_load4(L.p.beta, c, C, vec), mean = th_load4(L.p.mean, c, C, vec);
    const v4f invstd = th_load4(L.p.invstd, c, C, vec), dgamma = th_load4(L.p.dgamma, c, C, vec), dbeta = th_load4(L.p.dbeta, c, C, vec);
    const float Rf = (float)L.p.rows;
    v4f sf, c1, c2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sf[e] = gamma[e] * invstd[e]; c1[e] = __fdiv_rn(dbeta[e], Rf); c2[e] = __fdiv_rn(dgamma[e], Rf); }
    for (long long r = r0 + rl; r < r1; r += rpp) {
        const v4f x = th_load4(L.p.x + r * C, c, C, vec), dy = th_load4(L.p.dy + r * C, c, C, vec);
        v4f d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = x[e] - mean[e], xh = t * invstd[e];
            const float y = t * sf[e] + beta[e];
            const float gg = y > 0.0f ? dy[e] : 0.0f;
            const float u = gg - c1[e], v = xh * c2[e];
            d[e] = sf[e] * (u - v);
        }
        th_store4(L.p.out + r * C, c, C, vec, d);
    }
}

// slabs of a level list: about 1024 blocks in all, a slab a whole number of passes
static void make_slabs(StatArgs &a)
{
    a.CW = a.C < TH_STAT_COLS ? a.C : TH_STAT_COLS;
    const int G = (a.CW + 3) / 4, rpp = 256 / G;
    long long tot = 0;
    for (int l = 0; l < a.nlevels; ++l) tot += a.lv[l].p.rows;
    long long sr = (tot + 1023) / 1024;
    if (sr < 8LL * rpp) sr = 8LL * rpp;
    sr = (sr + rpp - 1) / rpp * rpp;
    a.slab_rows = (int)sr;
    int n = 0;
    for (int l = 0; l < a.nlevels; ++l) {
        a.lv[l].slab_begin = n;
        a.lv[l].n_slabs = (int)((a.lv[l].p.rows + sr - 1) / sr);
        n += a.lv[l].n_slabs;
    }
    a.n_slabs = n;
}

#define LAUNCH(kernel, grid, s, ...)                                  \
    do {                                                              \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, __VA_ARGS__); \
        HIPCHK(hipGetLastError());                                    \
    } while (0)

// ----------------------------------------------------------------------------- the convolutions
struct ConvTrainPlan {
    long long R[TH_MAX_LEVELS], roff[TH_MAX_LEVELS], Rtot;
    ConvW f, d;                         // geometry of the forward's and the data gradient's packed kernels (no pointers yet)
    int rows_per_slice, n_slices, slice_begin[TH_MAX_LEVELS], tiles_ci;
    StatArgs st;                        // dbias: the slabs of dy
    size_t off_a, off_b, off_w, off_bias, off_part, off_stat, bytes;
};

static const char *conv_plan(const ssd_conv_level *lv, int n, int B, int Cin, int Cout, ConvTrainPlan &p)
{
    if (!lv) return "null level list";
    if (n < 1 || n > TH_MAX_LEVELS) return "1 .. 8 levels";
    if (B < 1 || Cin < 1 || Cout < 1) return "sizes must be positive";
    if (Cin % 8) return "Cin must be a multiple of 8";
    if (Cin > 4096 || Cout > 4096) return "at most 4096 channels";
    conv_geometry(nullptr, 9, round_up(Cin, 32), round_up(Cout, 8), Cin, Cout, p.f);
    conv_geometry(nullptr, 9, round_up(Cout, 32), round_up(Cin, 8), Cout, Cin, p.d);
    const int widest = std::max(std::max(p.f.CinP, p.f.CoutP), std::max(p.d.CinP, p.d.CoutP));
    p.Rtot = 0;
    for (int l = 0; l < n; ++l) {
        if (lv[l].H < 1 || lv[l].W < 1) return "sizes must be positive";
        const long long R = (long long)B * lv[l].H * lv[l].W;
        if (lv[l].H > 32768 || lv[l].W > 32768 || R * widest * 4 >= (1LL << 31)) return "every level's tensors must stay below 2 GiB";
        p.R[l] = R;
        p.roff[l] = p.Rtot;
        p.Rtot += R;
    }
    if (p.Rtot >= (1LL << 31)) return "fewer than 2^31 positions in all";
    // K-slices of the weight gradient: about 1536 blocks in all
    p.tiles_ci = (Cin + 127) / 128;
    const int BN = wgrad_tile_n(Cout);
    const long long tiles = 9LL * p.tiles_ci * ((Cout + BN - 1) / BN);
    const long long want = std::max(1LL, 1536 / tiles);
    long long rps = (p.Rtot + want - 1) / want;
    if (rps < 256) rps = 256;
    rps = (rps + 15) / 16 * 16;
    p.rows_per_slice = (int)rps;
    p.n_slices = 0;
    for (int l = 0; l < n; ++l) {
        p.slice_begin[l] = p.n_slices;
        p.n_slices += (int)((p.R[l] + rps - 1) / rps);
    }
    memset(&p.st, 0, sizeof(p.st));
    p.st.nlevels = n;
    p.st.C = Cout;
    for (int l = 0; l < n; ++l) p.st.lv[l].p.rows = p.R[l];
    make_slabs(p.st);
    // workspace: [a | b | w | bias] of the forward or the data gradient, then the weight gradient's partial tiles and dbias's sums
    const size_t a_f = (size_t)p.Rtot * p.f.CinP, b_f = (size_t)p.Rtot * p.f.CoutP, w_f = (size_t)9 * p.f.CoutPad * p.f.CinP;
    const size_t a_d = (size_t)p.Rtot * p.d.CinP, b_d = (size_t)p.Rtot * p.d.CoutP, w_d = (size_t)9 * p.d.CoutPad * p.d.CinP;
    p.off_a = 0;
    p.off_b = al256(std::max(a_f, a_d) * 4 + 256);
    p.off_w = p.off_b + al256(std::max(b_f, b_d) * 4 + 256);
    p.off_bias = p.off_w + al256(std::max(w_f, w_d) * 4 + 256);
    p.off_part = p.off_bias + al256((size_t)p.f.CoutP * 4 + 256);
    p.off_stat = p.off_part + al256((size_t)p.n_slices * 9 * Cin * Cout * 4);
    p.bytes = p.off_stat + al256((size_t)p.st.n_slabs * 2 * Cout * 8);
    return nullptr;
}

static inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

extern "C" size_t ssd_conv3x3_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout)
{
    ConvTrainPlan p;
    return conv_plan(levels, n_levels, B, Cin, Cout, p) ? 0 : p.bytes;
}

static int run_igemm(const ConvW &cw, const float *in, float *out, const ssd_conv_level *lv, int n, int B, const ConvTrainPlan &p, hipStream_t s)
{
    std::vector<LevelDesc> ld;
    for (int l = 0; l < n; ++l)
        ld.push_back(dense_level(lv[l].H, lv[l].W, lv[l].H, lv[l].W, cw.CoutP, p.roff[l] * cw.CinP, p.roff[l] * cw.CoutP));
    ConvIO io{in, out};
    Op op = make_conv_op(nullptr, cw, io, B, 1, 1, SSD_ACT_NONE, ld, true);
    HIPCHK(op.run(s));
    return SSD_OK;
}

extern "C" int ssd_conv3x3_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                         const float *w_dev, const float *bias_dev, void *workspace_dev, size_t workspace_bytes,
                                         void *stream)
{
    ConvTrainPlan p;
    if (const char *why = conv_plan(levels, n_levels, B, Cin, Cout, p))
        return ssd_fail(SSD_ERR_INVALID, std::string("ssd_conv3x3_train_forward: ") + why);
    if (!w_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_forward: null pointer");
    if (mis16(w_dev) || mis16(workspace_dev) || ((uintptr_t)bias_dev & 3))
        return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_forward: w_dev and workspace_dev need 16-byte alignment, bias_dev 4-byte");
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l].x || !levels[l].out) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_forward: a level's x or out is null");
        if (mis16(levels[l].x) || mis16(levels[l].out)) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_forward: a level's x or out is not 16-byte aligned");
    }
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    float *xin = (float *)(ws + p.off_a), *outp = (float *)(ws + p.off_b), *wt = (float *)(ws + p.off_w), *biasp = (float *)(ws + p.off_bias);
    ConvW cw = p.f;
    for (int l = 0; l < n_levels; ++l)
        HIPCHK(launch_permute_channels(levels[l].x, p.R[l], Cin, cw.CinP, 1, xin + p.roff[l] * cw.CinP, s));
    const long long nw = 9LL * cw.CoutPad * cw.CinP;
    LAUNCH(pack_w_kernel, dim3((unsigned)((nw + 255) / 256)), s, w_dev, Cin, Cout, cw.CinP, cw.CoutPad, 0, wt);
    cw.wt = wt;
    if (bias_dev) {
        HIPCHK(launch_permute_channels(bias_dev, 1, Cout, cw.CoutP, 1, biasp, s));
        cw.bias = biasp;
    }
    SSDCHK(run_igemm(cw, xin, outp, levels, n_levels, B, p, s));
    for (int l = 0; l < n_levels; ++l)
        HIPCHK(launch_permute_channels(outp + p.roff[l] * cw.CoutP, p.R[l], Cout, cw.CoutP, 0, levels[l].out, s));
    return SSD_OK;
}

extern "C" int ssd_conv3x3_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                          const float *w_dev, float *dw_dev, float *dbias_dev, void *workspace_dev,
                                          size_t workspace_bytes, void *stream)
{
    ConvTrainPlan p;
    if (const char *why = conv_plan(levels, n_levels, B, Cin, Cout, p))
        return ssd_fail(SSD_ERR_INVALID, std::string("ssd_conv3x3_train_backward: ") + why);
    if (!w_dev || !dw_dev || !workspace_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: null pointer");
    if (mis16(w_dev) || mis16(dw_dev) || mis16(workspace_dev) || ((uintptr_t)dbias_dev & 3))
        return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: w_dev, dw_dev and workspace_dev need 16-byte alignment, dbias_dev 4-byte");
    int with_dx = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l].x || !levels[l].dy) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: a level's x or dy is null");
        if (mis16(levels[l].x) || mis16(levels[l].dy) || mis16(levels[l].out))
            return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: a level's x, dy or out is not 16-byte aligned");
        with_dx += levels[l].out ? 1 : 0;
    }
    if (with_dx != 0 && with_dx != n_levels)
        return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: dx (out) must be given for every level or for none");
    if (workspace_bytes < p.bytes) return ssd_fail(SSD_ERR_INVALID, "ssd_conv3x3_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    if (with_dx) {          // dx = conv3x3_same(dy, w'): the forward's launch on the rotated, transposed kernel
        float *dyp = (float *)(ws + p.off_a), *dxp = (float *)(ws + p.off_b), *wt = (float *)(ws + p.off_w);
        ConvW cw = p.d;
        for (int l = 0; l < n_levels; ++l)
            HIPCHK(launch_permute_channels(levels[l].dy, p.R[l], Cout, cw.CinP, 1, dyp + p.roff[l] * cw.CinP, s));
        const long long nw = 9LL * cw.CoutPad * cw.CinP;
        LAUNCH(pack_w_kernel, dim3((unsigned)((nw + 255) / 256)), s, w_dev, Cin, Cout, cw.CinP, cw.CoutPad, 1, wt);
        cw.wt = wt;
        SSDCHK(run_igemm(cw, dyp, dxp, levels, n_levels, B, p, s));
        for (int l = 0; l < n_levels; ++l)
            HIPCHK(launch_permute_channels(dxp + p.roff[l] * cw.CoutP, p.R[l], Cin, cw.CoutP, 0, levels[l].out, s));
    }
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.nlevels = n_levels; a.Cin = Cin; a.Cout = Cout;
    a.rows_per_slice = p.rows_per_slice; a.n_slices = p.n_slices; a.tiles_ci = p.tiles_ci;
    a.partial = (float *)(ws + p.off_part);
    for (int l = 0; l < n_levels; ++l) {
        WgradLevel &L = a.lv[l];
        L.x = levels[l].x; L.dy = levels[l].dy; L.H = levels[l].H; L.W = levels[l].W; L.R = (int)p.R[l];
        L.slice_begin = p.slice_begin[l];
        L.dHW = ssd_udiv_make((unsigned)(L.H * L.W));
        L.dW = ssd_udiv_make((unsigned)L.W);
    }
    HIPCHK(launch_wgrad(a, dw_dev, s));
    if (dbias_dev) {
        StatArgs st = p.st;
        st.partial = (double *)(ws + p.off_stat);
        for (int l = 0; l < n_levels; ++l) st.lv[l].p.x = levels[l].dy;
        st.lv[0].p.out = dbias_dev;
        LAUNCH(stat_partial<0>, dim3((unsigned)st.n_slabs, (unsigned)((Cout + TH_STAT_COLS - 1) / TH_STAT_COLS)), s, st);
        LAUNCH(stat_final<3>, dim3((unsigned)((Cout + 255) / 256), 1), s, st);
    }
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

extern "C" int ssd_bn_relu_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t training, float epsilon,
                                         float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    StatArgs a;
    if (const char *why = bn_plan(levels, n_levels, C, a)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_bn_relu_train_forward: ") + why);
    if (!(epsilon > 0.0f) || !(epsilon < 1e30f) || !(one_minus_momentum >= 0.0f) || !(one_minus_momentum <= 1.0f) || (training != 0 && training != 1))
        return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: epsilon > 0, 0 <= one_minus_momentum <= 1, training 0 or 1");
    for (int l = 0; l < n_levels; ++l) {
        const ssd_bn_level &L = levels[l];
        if (!L.x || !L.out || !L.gamma || !L.beta) return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: a level's x, out, gamma or beta is null");
        if (training ? (!L.mean || !L.invstd) : (!L.moving_mean || !L.moving_variance))
            return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: training needs mean and invstd, inference the moving statistics");
        if ((L.moving_mean == nullptr) != (L.moving_variance == nullptr))
            return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: the moving statistics must be given together");
        if (mis16(L.x) || mis16(L.out) || mis16(L.gamma) || mis16(L.beta) || mis16(L.moving_mean) || mis16(L.moving_variance) || mis16(L.mean) ||
            mis16(L.var) || mis16(L.invstd))
            return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: every pointer needs 16-byte alignment");
    }
    if (training && (!workspace_dev || mis16(workspace_dev))) return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: workspace_dev null or misaligned");
    if (training && workspace_bytes < al256((size_t)a.n_slabs * 2 * C * 8)) return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_forward: workspace too small");
    bn_fill(a, levels);
    a.partial = (double *)workspace_dev;
    a.eps = epsilon; a.one_minus_momentum = one_minus_momentum; a.training = training;
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

extern "C" int ssd_bn_relu_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, void *workspace_dev,
                                          size_t workspace_bytes, void *stream)
{
    StatArgs a;
    if (const char *why = bn_plan(levels, n_levels, C, a)) return ssd_fail(SSD_ERR_INVALID, std::string("ssd_bn_relu_train_backward: ") + why);
    for (int l = 0; l < n_levels; ++l) {
        const ssd_bn_level &L = levels[l];
        if (!L.x || !L.dy || !L.out || !L.gamma || !L.beta || !L.mean || !L.invstd || !L.dgamma || !L.dbeta)
            return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_backward: a level's x, dy, out, gamma, beta, mean, invstd, dgamma or dbeta is null");
        if (mis16(L.x) || mis16(L.dy) || mis16(L.out) || mis16(L.gamma) || mis16(L.beta) || mis16(L.mean) || mis16(L.invstd) || mis16(L.dgamma) ||
            mis16(L.dbeta))
            return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_backward: every pointer needs 16-byte alignment");
    }
    if (!workspace_dev || mis16(workspace_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_backward: workspace_dev null or misaligned");
    if (workspace_bytes < al256((size_t)a.n_slabs * 2 * C * 8)) return ssd_fail(SSD_ERR_INVALID, "ssd_bn_relu_train_backward: workspace too small");
    bn_fill(a, levels);
    a.partial = (double *)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(stat_partial<2>, dim3((unsigned)a.n_slabs), s, a);
    LAUNCH(stat_final<2>, dim3((unsigned)((C + 255) / 256), (unsigned)n_levels), s, a);
    LAUNCH(bn_apply_backward, dim3((unsigned)a.n_slabs), s, a);
    return SSD_OK;
}
