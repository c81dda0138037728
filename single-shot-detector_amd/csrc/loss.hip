// The EVAL loss on the GPU: matching (training_target_creation.py:48-130), targets (:133-176, box_utils.py:80-113) and the
// focal / smooth-L1 losses with their normalisation (losses.py, ssd.py:71-133).  Semantics and the tie rule:
// include/ssd_hip.h, block "the EVAL loss".
//
//   L1 best     per (image, chunk of 1 024 anchors): the image's gt in LDS, 4 anchors per thread; per gt the wave's best
//               key (iou bits << 32 | ~anchor: IoU >= 0, so key order == (IoU desc, anchor asc)) goes to an LDS 64-bit max,
//               the block's to one global 64-bit atomicMax per gt.  Order-independent: first index on ties.
//   L2 anchor   per (image, 64 anchors), 4 lanes per anchor: the lanes split the gt (g = q mod 4) for the per-anchor arg-max
//               and the forced overlay, combine through shuffles (first index on ties), write the optional targets; with
//               logits the 4 lanes split the anchor's C logits (16-byte loads when the rows are 16-byte aligned) into
//               double partial sums of the focal terms, and lane 0 adds the smooth-L1 term.  Per block: loc / cls sums in
//               double (fixed shuffle tree over the 64 anchors) and match counts per level into a slab.  No float atomics.
//   L3 sum      one block: per image the slab entries in a fixed order, per_image, then the batch in image order, losses.
//   L4 grad     ssd_loss_backward, one block per 256 rows (anchors of the flattened [B*N]): every wave first forms the
//               batch's normaliser from per_image[:,2] (integer counts, exact in double) and the two upstream gradients;
//               then the block writes the rows' d_codes (one row per thread) and streams their logits once, 4 per thread
//               in 16-byte loads / stores when C % 4 == 0 and the rows are 16-byte aligned, one per thread otherwise.
//               exp(-|x|) is formed once per logit and gives both sigma and log1p; every element is evaluated in double
//               and rounded once.  Each output element is written exactly once: no atomics, no clearing.
#include "host.h"

#include <cstring>

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

namespace {

constexpr int L1_THREADS = 256, L1_APT = 4, L1_TILE = 256;
constexpr int L2_THREADS = 256, L2_ANCHORS = 64, L2_TILE = 256;
constexpr int L3_THREADS = 256;
constexpr int L4_THREADS = 256, L4_ROWS = 256;
constexpr int32_t L4_MAX_C = 1 << 22;        // L4_ROWS * C elements of a block stay below 2^30: 32-bit offsets in a block
static_assert(L4_ROWS == L4_THREADS, "loss_grad writes one d_codes row per thread");

struct SlabEntry {             // one per (image, L2 block)
    double loc, cls;
    int32_t cnt[1 + SSD_LOSS_MAX_LEVELS];     // matches, matches per level
    int32_t pad;
};

struct LossArgs {
    const float *anchors, *gt_boxes, *logits, *codes;
    const int32_t *gt_labels, *gt_num;
    int32_t B, N, C, G;
    float pos_thr, neg_thr, gamma, alpha, one_m_alpha;
    int32_t n_levels;
    int64_t level_end[SSD_LOSS_MAX_LEVELS];
    float *reg_targets, *cls_losses, *loc_losses, *per_image, *losses;
    int32_t *cls_targets, *matches;
    u64 *keys;                 // [B,G] best anchor per gt (L1)
    SlabEntry *slab;           // [B, nblk]
    int32_t nblk;
};

__device__ __forceinline__ float area(const v4f b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// box_utils.py:14-66 for one pair, fp32 op by op: inter / ((area_gt + area_anchor) - inter + 1e-8), clipped to [0, 1]
__device__ __forceinline__ float iou(const v4f g, float ag, const v4f a, float aa)
{
    const float ih = fmaxf(0.0f, fminf(g[2], a[2]) - fmaxf(g[0], a[0]));
    const float iw = fmaxf(0.0f, fminf(g[3], a[3]) - fmaxf(g[1], a[1]));
    const float inter = ih * iw;
    const float uni = (ag + aa) - inter;
    const float v = inter / (uni + 1e-8f);
    return fminf(fmaxf(v, 0.0f), 1.0f);
}

__device__ __forceinline__ int n_gt(const LossArgs &p, int b)
{
    const int n = p.gt_num[b];
    return n < 0 ? 0 : (n > p.G ? p.G : n);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m)
{
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}

// ----------------------------------------------------------------------------- L1: best anchor per gt
__global__ __launch_bounds__(L1_THREADS) void loss_best_anchor(LossArgs p)
{
    __shared__ v4f s_box[L1_TILE];
    __shared__ float s_area[L1_TILE];
    __shared__ u64 s_best[L1_TILE];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int ng = n_gt(p, b);
    if (ng == 0) return;
    const int64_t a0 = (int64_t)blockIdx.x * (L1_THREADS * L1_APT);
    v4f an[L1_APT];
    float aa[L1_APT];
    int64_t ai[L1_APT];
    for (int j = 0; j < L1_APT; ++j) {
        ai[j] = a0 + j * L1_THREADS + t;
        an[j] = ai[j] < p.N ? *(const v4f *)(p.anchors + 4 * ai[j]) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
        aa[j] = area(an[j]);
    }
    const float *gb = p.gt_boxes + (int64_t)b * p.G * 4;
    for (int g0 = 0; g0 < ng; g0 += L1_TILE) {
        const int nt = min(L1_TILE, ng - g0);
        if (t < nt) {
            s_box[t] = *(const v4f *)(gb + 4 * (int64_t)(g0 + t));
            s_area[t] = area(s_box[t]);
            s_best[t] = 0;
        }
        __syncthreads();
        for (int g = 0; g < nt; ++g) {
            const v4f gbx = s_box[g];
            const float ag = s_area[g];
            u64 key = 0;
            for (int j = 0; j < L1_APT; ++j)
                if (ai[j] < p.N) {
                    const u64 k = ((u64)__float_as_uint(iou(gbx, ag, an[j], aa[j])) << 32) | (unsigned)~(unsigned)ai[j];
                    key = k > key ? k : key;
                }
            for (int m = 32; m >= 1; m >>= 1) {
                const u64 o = shfl_xor_u64(key, m);
                key = o > key ? o : key;
            }
            if (lane == 0 && key) atomicMax(&s_best[g], key);
        }
        __syncthreads();
        if (t < nt && s_best[t]) atomicMax(p.keys + (int64_t)b * p.G + g0 + t, s_best[t]);
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------- L2: per anchor
__device__ __forceinline__ float exp_cr(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log1p_cr(float x) { return (float)log1p((double)x); }
__device__ __forceinline__ float sigmoid_cr(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
__device__ __forceinline__ float log_cr(float x) { return (float)log((double)x); }

// losses.py:22-49 for one (anchor, class): z = 1 for the target class, 0 otherwise
__device__ __forceinline__ float focal_term(float x, bool z, const LossArgs &p)
{
    const float zf = z ? 1.0f : 0.0f;
    // sigmoid_cross_entropy_with_logits, TF r1.12: (relu(x) - x * z) + log1p(exp(-|x|))
    const float relu = x >= 0.0f ? x : 0.0f;
    const float nlpt = (relu - x * zf) + log1p_cr(exp_cr(-fabsf(x)));
    const float pr = sigmoid_cr(x);
    const float pt = z ? pr : 1.0f - pr;
    const float omp = 1.0f - pt;
    // tf.pow(1 - p_t, gamma) correctly rounded; for gamma == 2 the double square is exact, so one rounding is pow's
    const float mod = p.gamma == 2.0f ? (float)((double)omp * (double)omp) : (float)pow((double)omp, (double)p.gamma);
    const float w = z ? p.alpha * nlpt : p.one_m_alpha * nlpt;
    return mod * w;
}

__global__ __launch_bounds__(L2_THREADS) void loss_anchor(LossArgs p)
{
    __shared__ v4f s_box[L2_TILE];
    __shared__ float s_area[L2_TILE];
    __shared__ int32_t s_fa[L2_TILE];        // the gt's forced anchor, -1 - anchor when its IoU is < 0.1 (masked)
    __shared__ double s_red[2][L2_ANCHORS];
    __shared__ int32_t s_lvl[L2_ANCHORS];
    const int b = blockIdx.y, t = threadIdx.x, q = t & 3, al = t >> 2;
    const int64_t a = (int64_t)blockIdx.x * L2_ANCHORS + al;
    const bool live = a < p.N;
    const int ng = n_gt(p, b);
    const v4f an = live ? *(const v4f *)(p.anchors + 4 * a) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
    const float aa = area(an);
    // per-anchor arg-max over this lane's gt (g = q mod 4), strict > keeps the first index
    float best = -1.0f;
    int bi = 0x7fffffff, frow = 0x7fffffff, fok = 0;
    const float *gb = p.gt_boxes + (int64_t)b * p.G * 4;
    const u64 *keys = p.keys + (int64_t)b * p.G;
    for (int g0 = 0; g0 < ng; g0 += L2_TILE) {
        const int nt = min(L2_TILE, ng - g0);
        __syncthreads();
        if (t < nt) {
            s_box[t] = *(const v4f *)(gb + 4 * (int64_t)(g0 + t));
            s_area[t] = area(s_box[t]);
            const u64 k = keys[g0 + t];
            const int fa = (int)~(unsigned)(k & 0xffffffffu);
            s_fa[t] = __uint_as_float((unsigned)(k >> 32)) >= 0.1f ? fa : -1 - fa;      // training_target_creation.py:113-115
        }
        __syncthreads();
        if (live)
            for (int g = q; g < nt; g += 4) {
                const float v = iou(s_box[g], s_area[g], an, aa);
                if (v > best) { best = v; bi = g0 + g; }
                const int fa = s_fa[g];
                if (fa == a || -1 - fa == a) {
                    frow = min(frow, g0 + g);
                    fok |= fa == a;
                }
            }
    }
    // combine the 4 lanes of the anchor: larger IoU, then smaller index
    for (int m = 1; m <= 2; m <<= 1) {
        const float ob = __shfl_xor(best, m);
        const int oi = __shfl_xor(bi, m), orow = __shfl_xor(frow, m), ook = __shfl_xor(fok, m);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        frow = min(frow, orow);
        fok |= ook;
    }
    int match = -1;
    if (ng > 0) {
        if (best >= p.pos_thr) match = bi;
        else if (p.pos_thr != p.neg_thr && !(p.neg_thr > best)) match = -2;
        if (fok) match = frow;                                                              // :117-118
    }
    // create_targets (:133-176) + encode (box_utils.py:80-113)
    int label = 0;
    v4f tgt = {0.0f, 0.0f, 0.0f, 0.0f};
    if (match >= 0) {
        const v4f g = *(const v4f *)(gb + 4 * (int64_t)match);
        label = p.gt_labels[(int64_t)b * p.G + match] + 1;
        float ha = an[2] - an[0], wa = an[3] - an[1];
        const float cya = an[0] + 0.5f * ha, cxa = an[1] + 0.5f * wa;
        float h = g[2] - g[0], w = g[3] - g[1];
        const float cy = g[0] + 0.5f * h, cx = g[1] + 0.5f * w;
        ha += 1e-8f; wa += 1e-8f; h += 1e-8f; w += 1e-8f;
        tgt[0] = (cy - cya) / ha * 10.0f;
        tgt[1] = (cx - cxa) / wa * 10.0f;
        tgt[2] = log_cr(h / ha) * 5.0f;
        tgt[3] = log_cr(w / wa) * 5.0f;
    }
    const int64_t row = (int64_t)b * p.N + a;
    if (live && q == 0) {
        if (p.matches) p.matches[row] = match;
        if (p.cls_targets) p.cls_targets[row] = label;
        if (p.reg_targets) *(v4f *)(p.reg_targets + 4 * row) = tgt;
    }
    if (!p.logits) return;

    // focal loss over the anchor's C logits, lanes across classes
    double s = 0.0;
    if (live) {
        const float *lg = p.logits + row * p.C;
        const int tc = label - 1;                  // the target class (-1: none)
        if ((p.C & 3) == 0 && (((uintptr_t)p.logits) & 15) == 0) {
            for (int c = 4 * q; c < p.C; c += 16) {
                const v4f x = *(const v4f *)(lg + c);
                for (int k = 0; k < 4; ++k) s += (double)focal_term(x[k], c + k == tc, p);
            }
        } else {
            for (int c = q; c < p.C; c += 4) s += (double)focal_term(lg[c], c == tc, p);
        }
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    float cls = 0.0f, loc = 0.0f;
    if (live) {
        cls = (match >= -1 ? 1.0f : 0.0f) * (float)s;                                      // ssd.py:97-106
        const v4f c = *(const v4f *)(p.codes + 4 * row);
        double ls = 0.0;
        for (int k = 0; k < 4; ++k) {                                                       // losses.py:4-19
            const float d = fabsf(c[k] - tgt[k]);
            ls += (double)(d < 1.0f ? 0.5f * (d * d) : d - 0.5f);
        }
        loc = (match >= 0 ? 1.0f : 0.0f) * (float)ls;
        if (q == 0) {
            if (p.cls_losses) p.cls_losses[row] = cls;
            if (p.loc_losses) p.loc_losses[row] = loc;
        }
    }
    if (q == 0) {
        s_red[0][al] = (double)loc;
        s_red[1][al] = (double)cls;
        int lv = -1;
        if (live && match >= 0) {
            lv = 0;
            while (lv < p.n_levels - 1 && a >= p.level_end[lv]) ++lv;
        }
        s_lvl[al] = lv;
    }
    __syncthreads();
    if (t < 64) {                  // one wave: fixed shuffle tree over the block's 64 anchors
        double l = s_red[0][t], c = s_red[1][t];
        for (int m = 1; m < 64; m <<= 1) {
            l += __shfl_xor(l, m);
            c += __shfl_xor(c, m);
        }
        const int lv = s_lvl[t];
        const int tot = __popcll(__ballot(lv >= 0));
        int cnt[SSD_LOSS_MAX_LEVELS];
        for (int k = 0; k < SSD_LOSS_MAX_LEVELS; ++k) cnt[k] = __popcll(__ballot(lv == k && k < p.n_levels));
        if (t == 0) {
            SlabEntry &e = p.slab[(int64_t)b * p.nblk + blockIdx.x];
            e.loc = l;
            e.cls = c;
            e.cnt[0] = tot;
            for (int k = 0; k < SSD_LOSS_MAX_LEVELS; ++k) e.cnt[1 + k] = cnt[k];
        }
    }
}

// ----------------------------------------------------------------------------- L3: fixed-order sums
__global__ __launch_bounds__(L3_THREADS) void loss_sum(LossArgs p)
{
    __shared__ double s_d[2][L3_THREADS];
    __shared__ int64_t s_c[1 + SSD_LOSS_MAX_LEVELS][L3_THREADS];
    const int t = threadIdx.x;
    double tot_loc = 0.0, tot_cls = 0.0;
    int64_t tot_cnt = 0;
    const int w = 3 + p.n_levels;
    for (int b = 0; b < p.B; ++b) {
        double l = 0.0, c = 0.0;
        int64_t n[1 + SSD_LOSS_MAX_LEVELS] = {};
        for (int k = t; k < p.nblk; k += L3_THREADS) {
            const SlabEntry &e = p.slab[(int64_t)b * p.nblk + k];
            l += e.loc;
            c += e.cls;
            for (int j = 0; j <= SSD_LOSS_MAX_LEVELS; ++j) n[j] += e.cnt[j];
        }
        s_d[0][t] = l;
        s_d[1][t] = c;
        for (int j = 0; j <= SSD_LOSS_MAX_LEVELS; ++j) s_c[j][t] = n[j];
        __syncthreads();
        for (int h = L3_THREADS / 2; h > 0; h >>= 1) {
            if (t < h) {
                s_d[0][t] += s_d[0][t + h];
                s_d[1][t] += s_d[1][t + h];
                for (int j = 0; j <= SSD_LOSS_MAX_LEVELS; ++j) s_c[j][t] += s_c[j][t + h];
            }
            __syncthreads();
        }
        if (t == 0) {
            if (p.per_image) {
                float *o = p.per_image + (int64_t)b * w;
                o[0] = (float)s_d[0][0];
                o[1] = (float)s_d[1][0];
                o[2] = (float)s_c[0][0];
                for (int j = 0; j < p.n_levels; ++j) o[3 + j] = (float)s_c[1 + j][0];
            }
            tot_loc += s_d[0][0];
            tot_cls += s_d[1][0];
            tot_cnt += s_c[0][0];
        }
        __syncthreads();
    }
    if (t == 0 && p.losses) {
        const float norm = fmaxf((float)tot_cnt, 1.0f);                                    // ssd.py:120-123
        p.losses[0] = (float)tot_loc / norm;
        p.losses[1] = (float)tot_cls / norm;
    }
}

// ----------------------------------------------------------------------------- L4: the gradient (ssd_loss_backward)
struct GradArgs {
    const float *logits, *codes, *reg_targets, *per_image, *grad;
    const int32_t *cls_targets, *matches;
    float *d_logits, *d_codes;
    int64_t rows;              // B * N
    int32_t B, C, stride;
    double gamma, alpha, one_m_alpha;
    int32_t vec;               // C % 4 == 0 and logits / d_logits 16-byte aligned
};

// g / norm for (localization, classification); norm = max(sum of per_image[:,2], 1) in fp32, the value L3 divides by.
// The counts are integers: the double sum is exact in any order.  Every wave forms it itself (no barrier).
__device__ __forceinline__ void grad_scales(const GradArgs &p, double &gl, double &gc)
{
    const int lane = threadIdx.x & 63;
    double n = 0.0;
    for (int b = lane; b < p.B; b += 64) n += (double)p.per_image[(int64_t)b * p.stride + 2];
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    const double norm = (double)fmaxf((float)n, 1.0f);
    gl = (p.grad ? (double)p.grad[0] : 1.0) / norm;
    gc = (p.grad ? (double)p.grad[1] : 1.0) / norm;
}

// d focal / dx for one (anchor, class), z = 1 for the target class (include/ssd_hip.h, ssd_loss_backward):
// alpha_z * (gamma * q^(gamma-1) * dq/dx * nlp + q^gamma * (s - z)) * gc, in double, rounded once.  s and 1 - s both come
// from e = exp(-|x|) without cancellation: s = 1 / (1 + e) for x >= 0, e / (1 + e) otherwise.
__device__ __forceinline__ float focal_grad(float x, bool z, const GradArgs &p, double gc)
{
    const double xd = x;
    const double e = exp(-fabs(xd));
    const double r = 1.0 / (1.0 + e);
    const double s = xd >= 0.0 ? r : e * r, sc = xd >= 0.0 ? e * r : r;           // sigma(x), 1 - sigma(x)
    const double nlp = ((xd >= 0.0 ? xd : 0.0) - (z ? xd : 0.0)) + log1p(e);
    const double q = z ? sc : s;
    const double dq = z ? -(s * sc) : s * sc;
    const double smz = z ? -sc : s;                                                  // s - z
    double t1, qg;
    if (p.gamma == 2.0) {
        t1 = 2.0 * q * dq * nlp;
        qg = q * q;
    } else {
        // gamma * q^(gamma-1) * dq/dx with dq/dx = +-q(1-q) folded in: gamma * q^gamma * (+-(1-q)).  No q^(gamma-1): for
        // gamma < 1 it overflows on a denormal q (gamma == 0: 0 * inf) and has no value at q == 0; this form is 0 there
        qg = pow(q, p.gamma);
        t1 = p.gamma * qg * (z ? -s : sc) * nlp;
    }
    return (float)((z ? p.alpha : p.one_m_alpha) * (t1 + qg * smz) * gc);
}

__global__ __launch_bounds__(L4_THREADS) void loss_grad(GradArgs p)
{
    double gl, gc;
    grad_scales(p, gl, gc);
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * L4_ROWS;
    const int nr = (int)min((int64_t)L4_ROWS, p.rows - r0);
    if (t < nr) {                                                                    // d_codes: smooth-L1
        const int64_t r = r0 + t;
        v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.matches[r] >= 0) {
            const v4f c = *(const v4f *)(p.codes + 4 * r), g = *(const v4f *)(p.reg_targets + 4 * r);
            for (int k = 0; k < 4; ++k) {
                const float df = c[k] - g[k];
                const float v = fabsf(df) < 1.0f ? df : (df > 0.0f ? 1.0f : -1.0f);
                d[k] = (float)((double)v * gl);
            }
        }
        *(v4f *)(p.d_codes + 4 * r) = d;
    }
    const uint32_t C = (uint32_t)p.C, ne = (uint32_t)nr * C;
    const float *lg = p.logits + r0 * p.C;
    float *dl = p.d_logits + r0 * p.C;
    if (p.vec) {
        for (uint32_t j = 4 * t; j < ne; j += 4 * L4_THREADS) {
            const uint32_t rr = j / C;
            const int64_t r = r0 + rr;
            v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
            if (p.matches[r] >= -1) {
                const int tc = (int)(p.cls_targets[r] - 1) - (int)(j - rr * C);     // the target class, relative to j
                const v4f x = *(const v4f *)(lg + j);
                for (int k = 0; k < 4; ++k) d[k] = focal_grad(x[k], k == tc, p, gc);
            }
            *(v4f *)(dl + j) = d;
        }
    } else {
        for (uint32_t j = t; j < ne; j += L4_THREADS) {
            const uint32_t rr = j / C;
            const int64_t r = r0 + rr;
            float d = 0.0f;
            if (p.matches[r] >= -1) d = focal_grad(lg[j], (int)(j - rr * C) == p.cls_targets[r] - 1, p, gc);
            dl[j] = d;
        }
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int32_t l2_blocks(int32_t N) { return (N + L2_ANCHORS - 1) / L2_ANCHORS; }

size_t workspace_bytes(int32_t B, int32_t N, int32_t G)
{
    return align256((size_t)B * (size_t)(G > 0 ? G : 1) * sizeof(u64)) + align256((size_t)B * l2_blocks(N) * sizeof(SlabEntry));
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

int prepare(LossArgs &p, const char *who, const float *anchors, int32_t N, const float *gt_boxes, const int32_t *gt_labels,
            const int32_t *gt_num, int32_t B, int32_t G, const ssd_loss_config *cfg, void *ws, size_t ws_bytes)
{
    const std::string w(who);
    if (!anchors || (G > 0 && (!gt_boxes || !gt_labels)) || !gt_num || !cfg || !ws || B < 1 || N < 1 || G < 0)
        return ssd_fail(SSD_ERR_INVALID, w + ": bad arguments");
    if (G > SSD_LOSS_MAX_GT) return ssd_fail(SSD_ERR_INVALID, w + ": more than SSD_LOSS_MAX_GT (4096) groundtruth boxes per image");
    if ((int64_t)B * N * 4 >= ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, w + ": tensors too large");
    if (!aligned16(anchors) || !aligned16(gt_boxes) || !aligned16(ws)) return ssd_fail(SSD_ERR_INVALID, w + ": anchors, gt_boxes and the workspace must be 16-byte aligned");
    if (ws_bytes < workspace_bytes(B, N, G)) return ssd_fail(SSD_ERR_INVALID, w + ": workspace too small");
    if (!(cfg->positives_threshold >= cfg->negatives_threshold))                           // training_target_creation.py:87
        return ssd_fail(SSD_ERR_INVALID, w + ": positives_threshold < negatives_threshold");
    memset(&p, 0, sizeof(p));
    p.anchors = anchors; p.gt_boxes = gt_boxes; p.gt_labels = gt_labels; p.gt_num = gt_num;
    p.B = B; p.N = N; p.G = G;
    p.pos_thr = cfg->positives_threshold; p.neg_thr = cfg->negatives_threshold;
    p.keys = (u64 *)ws;
    p.slab = (SlabEntry *)((char *)ws + align256((size_t)B * (size_t)(G > 0 ? G : 1) * sizeof(u64)));
    p.nblk = l2_blocks(N);
    return SSD_OK;
}

hipError_t launch(const LossArgs &p, bool sum, hipStream_t s)
{
    if (p.G > 0) {
        hipError_t e = hipMemsetAsync(p.keys, 0, (size_t)p.B * p.G * sizeof(u64), s);
        if (e != hipSuccess) return e;
        const int per = L1_THREADS * L1_APT;
        hipLaunchKernelGGL(loss_best_anchor, dim3((p.N + per - 1) / per, p.B), dim3(L1_THREADS), 0, s, p);
    }
    hipLaunchKernelGGL(loss_anchor, dim3(p.nblk, p.B), dim3(L2_THREADS), 0, s, p);
    if (sum) hipLaunchKernelGGL(loss_sum, dim3(1), dim3(L3_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t ssd_loss_workspace_bytes(int32_t B, int32_t N, int32_t G)
{
    if (B < 1 || N < 1 || G < 0) return 0;
    return workspace_bytes(B, N, G);
}

extern "C" int ssd_training_targets(const float *anchors_dev, int32_t N, const float *gt_boxes_dev, const int32_t *gt_labels_dev,
                                    const int32_t *gt_num_dev, int32_t B, int32_t G, const ssd_loss_config *cfg,
                                    float *reg_targets_dev, int32_t *cls_targets_dev, int32_t *matches_dev,
                                    void *workspace_dev, size_t workspace_bytes, void *stream)
{
    LossArgs p;
    SSDCHK(prepare(p, "ssd_training_targets", anchors_dev, N, gt_boxes_dev, gt_labels_dev, gt_num_dev, B, G, cfg, workspace_dev,
                   workspace_bytes));
    if (reg_targets_dev && !aligned16(reg_targets_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_training_targets: reg_targets must be 16-byte aligned");
    p.reg_targets = reg_targets_dev; p.cls_targets = cls_targets_dev; p.matches = matches_dev;
    HIPCHK(launch(p, false, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" int ssd_loss(const float *logits_dev, const float *codes_dev, const float *anchors_dev, int32_t B, int32_t N, int32_t C,
                        const float *gt_boxes_dev, const int32_t *gt_labels_dev, const int32_t *gt_num_dev, int32_t G,
                        const ssd_loss_config *cfg, float *per_image_dev, float *losses_dev, float *cls_losses_dev,
                        float *loc_losses_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    LossArgs p;
    SSDCHK(prepare(p, "ssd_loss", anchors_dev, N, gt_boxes_dev, gt_labels_dev, gt_num_dev, B, G, cfg, workspace_dev,
                   workspace_bytes));
    if (!logits_dev || !codes_dev || C < 1) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: bad arguments");
    if ((int64_t)B * N * C >= ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: tensors too large");
    if (!aligned16(codes_dev)) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: codes must be 16-byte aligned");
    if (cfg->n_levels < 0 || cfg->n_levels > SSD_LOSS_MAX_LEVELS) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: n_levels out of range");
    int64_t end = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        if (cfg->anchors_per_level[l] < 0) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: negative anchors_per_level");
        end += cfg->anchors_per_level[l];
        p.level_end[l] = end;
    }
    if (cfg->n_levels > 0 && end != N) return ssd_fail(SSD_ERR_INVALID, "ssd_loss: anchors_per_level does not sum to N");
    p.logits = logits_dev; p.codes = codes_dev; p.C = C;
    p.gamma = cfg->gamma;
    p.alpha = (float)cfg->alpha;
    p.one_m_alpha = (float)(1.0 - cfg->alpha);
    p.n_levels = cfg->n_levels;
    p.per_image = per_image_dev; p.losses = losses_dev; p.cls_losses = cls_losses_dev; p.loc_losses = loc_losses_dev;
    HIPCHK(launch(p, true, (hipStream_t)stream));
    return SSD_OK;
}

extern "C" int ssd_loss_backward(const float *logits_dev, const float *codes_dev, int32_t B, int32_t N, int32_t C,
                                 const float *reg_targets_dev, const int32_t *cls_targets_dev, const int32_t *matches_dev,
                                 const float *per_image_dev, int32_t per_image_stride, const ssd_loss_config *cfg,
                                 const float *grad_losses_dev, float *d_logits_dev, float *d_codes_dev, void *stream)
{
    if (!logits_dev || !codes_dev || !reg_targets_dev || !cls_targets_dev || !matches_dev || !per_image_dev || !cfg ||
        !d_logits_dev || !d_codes_dev || B < 1 || N < 1 || C < 1 || per_image_stride < 3)
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_backward: bad arguments");
    if (C > L4_MAX_C) return ssd_fail(SSD_ERR_INVALID, "ssd_loss_backward: more than 4194304 classes");
    if ((int64_t)B * N * 4 >= ((int64_t)1 << 40) || (int64_t)B * N * C >= ((int64_t)1 << 40))
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_backward: tensors too large");
    if (!aligned16(codes_dev) || !aligned16(reg_targets_dev) || !aligned16(d_codes_dev))
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_backward: codes, reg_targets and d_codes must be 16-byte aligned");
    const void *word[] = {logits_dev, d_logits_dev, cls_targets_dev, matches_dev, per_image_dev, grad_losses_dev};
    for (const void *w : word)
        if ((uintptr_t)w & 3) return ssd_fail(SSD_ERR_INVALID, "ssd_loss_backward: misaligned pointer");
    GradArgs p;
    memset(&p, 0, sizeof(p));
    p.logits = logits_dev; p.codes = codes_dev; p.reg_targets = reg_targets_dev; p.per_image = per_image_dev;
    p.grad = grad_losses_dev; p.cls_targets = cls_targets_dev; p.matches = matches_dev;
    p.d_logits = d_logits_dev; p.d_codes = d_codes_dev;
    p.rows = (int64_t)B * N; p.B = B; p.C = C; p.stride = per_image_stride;
    p.gamma = (double)cfg->gamma;                                                    // the constants of L2 (focal_term)
    p.alpha = (double)(float)cfg->alpha;
    p.one_m_alpha = (double)(float)(1.0 - cfg->alpha);
    p.vec = (C & 3) == 0 && aligned16(logits_dev) && aligned16(d_logits_dev);
    const int64_t blocks = (p.rows + L4_ROWS - 1) / L4_ROWS;
    hipLaunchKernelGGL(loss_grad, dim3((unsigned)blocks), dim3(L4_THREADS), 0, (hipStream_t)stream, p);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
