// ssd_finalize's work: the reference's TF variables (by name) -> the packed device weights of the HIP kernels:
// physical channel order and padding (ssd_internal.h), transposed [tap][CoutPad][Cin] conv kernels (+ their split-fp16
// form for precision mode f16x3), batch-norm scale factors, slice-major depthwise packs.
#include "host.h"

#include <cmath>
#include <cstdio>
#include <cstring>

// physical position p -> logical channel (or -1 for a pad channel)
std::vector<int> phys_map(int C, int Cp)
{
    std::vector<int> m(Cp);
    for (int p = 0; p < Cp; ++p) {
        int l = ssd_logical_of_phys(p);
        m[p] = l < C ? l : -1;
    }
    return m;
}
std::vector<int> ident_map(int C, int Cp)
{
    std::vector<int> m(Cp);
    for (int p = 0; p < Cp; ++p) m[p] = p < C ? p : -1;
    return m;
}

std::vector<int> twopart_map(int D, int Dp)
{
    std::vector<int> m(2 * Dp, -1);
    for (int part = 0; part < 2; ++part)
        for (int p = 0; p < Dp; ++p) {
            const int l = ssd_logical_of_phys(p);
            if (l < D) m[part * Dp + p] = part * D + l;
        }
    return m;
}

// rows [rows][C] in logical channel order -> [rows][map.size()] in the order of `map`, pad channels zero: THE place where a
// weight tensor takes the physical channel order (ssd_internal.h); the width and the map are the caller's
std::vector<float> permute_rows(const float *w, int rows, int C, const std::vector<int> &map)
{
    const size_t Cp = map.size();
    std::vector<float> t((size_t)rows * Cp, 0.0f);
    for (int r = 0; r < rows; ++r)
        for (size_t p = 0; p < Cp; ++p)
            if (map[p] >= 0) t[r * Cp + p] = w[(size_t)r * C + map[p]];
    return t;
}

// ... and a batch norm's three vectors, appended to `o` (mean == nullptr, a layer without batch norm: nothing)
BnHost permute_bn(const float *mean, const float *sf, const float *beta, const std::vector<int> &map, BnHost o)
{
    if (!mean) return o;
    for (int p : map) {
        o.mean.push_back(p < 0 ? 0.f : mean[p]);
        o.sf.push_back(p < 0 ? 0.f : sf[p]);
        o.beta.push_back(p < 0 ? 0.f : beta[p]);
    }
    return o;
}

// batch_norm_relu (layer_utils.py:5-12): sf = gamma * rsqrt(var + 1e-3); appended to `o` (the head towers: one batch norm per level)
static void bn_pack(const float *gamma, const float *beta, const float *mean, const float *var, int C,
                    const std::vector<int> &outmap, BnHost &o)
{
    const float eps = 1e-3f;
    std::vector<float> sf(C);
    for (int c = 0; c < C; ++c) {
        float s = 1.0f / sqrtf(var[c] + eps);
        sf[c] = gamma[c] * s;
    }
    o = permute_bn(mean, sf.data(), beta, outmap, std::move(o));
}

static int pick_tile(const ssd_handle *h, int CoutP)
{
    if (CoutP <= 32) return IGEMM_128x32;
    if (CoutP <= 64) return IGEMM_128x64;
    // an output width that 96 divides but 128 does not (the 480 = 6 x 80 class logits): no padded columns
    // (option igemm_96 = 0 keeps the padded 128-wide tiles: tests / A-B runs)
    if (ssd_opt(h, OPT_IGEMM_96, 1) && CoutP % 128 != 0 && CoutP % 96 == 0) return IGEMM_128x96;
    return IGEMM_128x128;
}

// The geometry of a packed kernel of these padded widths: what pack_conv fills below and what train_head.hip, which packs on the
// device, must agree with.  (g_force_tile: -1 in the shipped library; in the SSD_DIAG build non-negative only inside ssd_bench_conv.)
void conv_geometry(const ssd_handle *h, int taps, int CinP, int CoutP, int Cin_l, int Cout_l, ConvW &cw)
{
    cw.taps = taps;
    cw.CinP = CinP;
    cw.CoutP = CoutP;
    cw.tile = g_force_tile >= 0 ? g_force_tile : pick_tile(h, cw.CoutP);
    cw.CoutPad = round_up(cw.CoutP, igemm_tile_bn(cw.tile));
    cw.Cin_l = Cin_l;
    cw.Cout_l = Cout_l;
}

// w: HWIO [k,k,Cin_l,Cout_l] -> wt [taps][CoutPad][CinP]
// The screen's operands (logit_screen.hip) from the packed kernel t [taps][CoutPad][CinP]: Wp = max(w, 0) rounded UP to
// f16, Wn = max(-w, 0) rounded DOWN, neither ever subnormal (a positive value below 2^-14 becomes 2^-14 in Wp and 0 in Wn: the
// bound then holds whether or not the matrix pipe flushes subnormal inputs); a NaN weight goes to Wp, where it marks.
// For every (k, column) at most one of the two is non-zero, so both live in ONE signed plane [taps][NT * 128][CinP]: the bits of
// Wp where w > 0 or w is NaN, 0x8000 | Wn where Wn is non-zero, +0 everywhere else (never -0).  The kernel's waves take their
// operand back out of it with integer operations (screen_operand).
// cst[n] >= bias + 2^-14 * sum Wn + 2^-20 |bias| (the input plane's round-up to a normal half, the epilogue's one rounding).
static int pack_screen(DevPool &pool, const std::vector<float> &t, const float *bias, ConvW &cw)
{
    const int NT = (cw.CoutP + 127) / 128, rows = NT * 128;
    std::vector<uint16_t> s((size_t)cw.taps * rows * cw.CinP, 0);       // (+0 wherever neither is non-zero: -0 is never written)
    std::vector<double> wn_sum(cw.CoutP, 0.0);
    auto bits_of = [](_Float16 v) { uint16_t b; memcpy(&b, &v, 2); return b; };
    for (int tap = 0; tap < cw.taps; ++tap)
        for (int n = 0; n < cw.CoutP; ++n) {
            const float *src = &t[((size_t)tap * cw.CoutPad + n) * cw.CinP];
            uint16_t *dp = &s[((size_t)tap * rows + n) * cw.CinP];
            for (int p = 0; p < cw.CinP; ++p) {
                const float v = src[p];
                if (v != v) { dp[p] = 0x7e00; continue; }
                if (v > 0.0f) {
                    const _Float16 hh = (_Float16)v;
                    uint16_t b = bits_of(hh);
                    if ((float)hh < v) b += 1;
                    dp[p] = b < 0x0400 ? 0x0400 : b;
                } else if (v < 0.0f) {
                    const float m = -v;
                    const _Float16 hh = (_Float16)m;
                    uint16_t b = bits_of(hh);
                    if ((float)hh > m) b -= 1;
                    if (b >= 0x7c00) b = 0x7bff;
                    if (b < 0x0400) b = 0;
                    dp[p] = b ? (uint16_t)(0x8000 | b) : 0;
                    _Float16 back;
                    memcpy(&back, &b, 2);
                    wn_sum[n] += (double)(float)back;
                }
            }
        }
    std::vector<float> cst(cw.CoutP);
    for (int n = 0; n < cw.CoutP; ++n) {
        const double b = bias[n];
        const double c = b + ldexp(wn_sum[n] * (1.0 + 1e-9), -14) + ldexp(fabs(b), -20) + 1e-30;
        float f = (float)c;
        if ((double)f < c) f = nextafterf(f, INFINITY);
        cst[n] = f;
    }
    SSDCHK(pool.upload(&cw.wscr, s));
    return pool.upload(&cw.scst, cst);
}

int pack_conv(const ssd_handle *h, DevPool &pool, const float *w, int k, int Cin_l, int Cout_l, const std::vector<int> &inmap,
                     const std::vector<int> &outmap, ConvW &cw, const float *screen_bias)
{
    conv_geometry(h, k * k, (int)inmap.size(), (int)outmap.size(), Cin_l, Cout_l, cw);
    std::vector<float> t((size_t)cw.taps * cw.CoutPad * cw.CinP, 0.0f);
    for (int tap = 0; tap < cw.taps; ++tap)
        for (int n = 0; n < cw.CoutP; ++n) {
            if (outmap[n] < 0) continue;
            float *dst = &t[((size_t)tap * cw.CoutPad + n) * cw.CinP];
            for (int p = 0; p < cw.CinP; ++p)
                if (inmap[p] >= 0) dst[p] = w[((size_t)tap * Cin_l + inmap[p]) * Cout_l + outmap[n]];
        }
    SSDCHK(pool.upload(&cw.wt, t));
    if (screen_bias && cw.taps == 9 && cw.CinP % 64 == 0 && cw.CoutP % 8 == 0 && cw.CoutP == Cout_l) SSDCHK(pack_screen(pool, t, screen_bias, cw));
    {   // igemm_lat.hip: per (tap, 16-channel tile, K-step of 32 channels) two 1-KB pieces in MFMA lane order -- lane
        // (i = l & 15, kk = l >> 4) holds the weights of channel row i for k = 4 t + kk, t = 4 hf .. 4 hf + 3
        const int KC = cw.CinP / 32, NT = cw.CoutPad / 16;
        std::vector<float> wl(t.size());
        for (int tap = 0; tap < cw.taps; ++tap)
            for (int ct = 0; ct < NT; ++ct)
                for (int kc = 0; kc < KC; ++kc)
                    for (int hf = 0; hf < 2; ++hf)
                        for (int l = 0; l < 64; ++l)
                            for (int e = 0; e < 4; ++e) {
                                const int i = l & 15, kk = l >> 4, cl = 4 * (4 * hf + e) + kk;      // logical channel within the K-step
                                const int phys = kc * 32 + ssd_phys_of_logical(cl);
                                wl[((((size_t)(tap * NT + ct) * KC + kc) * 2 + hf) * 64 + l) * 4 + e] =
                                    t[((size_t)tap * cw.CoutPad + ct * 16 + i) * cw.CinP + phys];
                            }
        SSDCHK(pool.upload(&cw.wlat, wl));
    }
    // split-fp16 rows of w * 2^s (igemm.hip "S16"): per octet of 8 input channels 8 halves h, then 8 halves
    // l = f16(w*2^s - h).  s puts the largest magnitude into [2^8, 2^9): every l of a weight within 2^-10 of
    // the largest is a normal half, and the scale is undone exactly in the epilogue (acc * 2^-s).
    float mx = 0.0f;
    for (float v : t) mx = fmaxf(mx, fabsf(v));
    int sh = 0;
    if (mx > 0.0f && std::isfinite(mx)) sh = 8 - ilogbf(mx);
    sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
    cw.scale16 = ldexpf(1.0f, -sh);
    std::vector<uint16_t> t16(t.size() * 2);
    for (size_t r = 0; r < t.size() / 8; ++r)
        for (int e = 0; e < 8; ++e) {
            const float x = ldexpf(t[r * 8 + e], sh);
            const _Float16 hh = (_Float16)x;
            const _Float16 ll = (_Float16)(x - (float)hh);
            memcpy(&t16[r * 16 + e], &hh, 2);
            memcpy(&t16[r * 16 + 8 + e], &ll, 2);
        }
    uint16_t *d16 = nullptr;
    SSDCHK(pool.upload(&d16, t16));
    cw.wt16 = (float *)d16;
    cw.CoutPad16 = cw.CoutPad;
    if (cw.CoutP >= 256 && cw.CoutPad % 256 != 0) {
        cw.CoutPad16 = round_up(cw.CoutP, 256);
        const size_t rowh = (size_t)cw.CinP * 2;        // halves per row
        std::vector<uint16_t> w16((size_t)cw.taps * cw.CoutPad16 * rowh, 0);
        for (int tap = 0; tap < cw.taps; ++tap)
            memcpy(&w16[(size_t)tap * cw.CoutPad16 * rowh], &t16[(size_t)tap * cw.CoutPad * rowh], (size_t)cw.CoutPad * rowh * 2);
        uint16_t *dw = nullptr;
        SSDCHK(pool.upload(&dw, w16));
        cw.wt16w = (float *)dw;
    }
    return SSD_OK;
}

int upload_bn(DevPool &pool, const BnHost &b, ConvW &cw)
{
    SSDCHK(pool.upload(&cw.mean, b.mean));
    SSDCHK(pool.upload(&cw.sf, b.sf));
    return pool.upload(&cw.beta, b.beta);
}

// slice-major copy of a depthwise layer's parameters for the streaming fused kernel (which always has a batch norm)
int pack_dw(DevPool &pool, const std::vector<float> &w9, const BnHost &b, DwW &d)
{
    if (d.Cp % 32 || b.mean.empty()) return SSD_OK;
    const int KC = d.Cp / 32;
    std::vector<float> p((size_t)KC * 12 * 32);
    for (int s = 0; s < KC; ++s)
        for (int c = 0; c < 32; ++c) {
            for (int t = 0; t < 9; ++t) p[((size_t)s * 12 + t) * 32 + c] = w9[(size_t)t * d.Cp + s * 32 + c];
            p[((size_t)s * 12 + 9) * 32 + c] = b.mean[s * 32 + c];
            p[((size_t)s * 12 + 10) * 32 + c] = b.sf[s * 32 + c];
            p[((size_t)s * 12 + 11) * 32 + c] = b.beta[s * 32 + c];
        }
    return pool.upload(&d.pack, p);
}

// a depthwise layer's (9 taps) or a first convolution's (27) rows over d.Cp channels and its batch norm: one upload per non-empty
// vector (a stage call may come without batch norm), and behind nine taps the pack
int upload_dw(DevPool &pool, const std::vector<float> &w, const BnHost &b, DwW &d)
{
    if (!w.empty()) SSDCHK(pool.upload(&d.w, w));
    if (!b.mean.empty()) SSDCHK(pool.upload(&d.mean, b.mean));
    if (!b.sf.empty()) SSDCHK(pool.upload(&d.sf, b.sf));
    if (!b.beta.empty()) SSDCHK(pool.upload(&d.beta, b.beta));
    return w.size() == (size_t)9 * d.Cp ? pack_dw(pool, w, b, d) : SSD_OK;
}

static const Tensor *getvar(ssd_handle *h, const std::string &n, std::initializer_list<int64_t> shape)
{
    auto it = h->vars.find(n);
    if (it == h->vars.end()) { ssd_fail(SSD_ERR_WEIGHT, "missing variable " + n); return nullptr; }
    const Tensor &t = it->second;
    std::vector<int64_t> want(shape);
    if (t.shape != want) {
        std::string s = "variable " + n + " has shape [";
        for (auto d : t.shape) s += std::to_string(d) + ",";
        s += "] expected [";
        for (auto d : want) s += std::to_string(d) + ",";
        ssd_fail(SSD_ERR_WEIGHT, s + "]");
        return nullptr;
    }
    return &t;
}

static int get_bn(ssd_handle *h, const std::string &scope, int C, const std::vector<int> &outmap, BnHost &o)
{
    const Tensor *g = getvar(h, scope + "/gamma", {C}), *b = getvar(h, scope + "/beta", {C});
    const Tensor *m = getvar(h, scope + "/moving_mean", {C}), *v = getvar(h, scope + "/moving_variance", {C});
    if (!g || !b || !m || !v) return SSD_ERR_WEIGHT;
    bn_pack(g->data.data(), b->data.data(), m->data.data(), v->data.data(), C, outmap, o);
    return SSD_OK;
}

// dense conv + optional BN, standard physical maps on both sides
// (in_split > 0: the input is a ShuffleNet stage output in two-part rows, in_split channels per half)
static int load_conv(ssd_handle *h, const std::string &wname, const std::string &bnscope, int k, int Cin, int Cout,
                     ConvW &cw, bool out_identity = false, int in_split = 0, const float *screen_bias = nullptr)
{
    const Tensor *w = getvar(h, wname, {k, k, Cin, Cout});
    if (!w) return SSD_ERR_WEIGHT;
    std::vector<int> inmap = in_split > 0 ? twopart_map(in_split, round_up(in_split, 32)) : phys_map(Cin, round_up(Cin, 32));
    std::vector<int> outmap = out_identity ? ident_map(Cout, Cout) : phys_map(Cout, round_up(Cout, 32));
    SSDCHK(pack_conv(h, h->wpool, w->data.data(), k, Cin, Cout, inmap, outmap, cw, out_identity ? screen_bias : nullptr));
    if (!bnscope.empty()) {
        BnHost b;
        SSDCHK(get_bn(h, bnscope, Cout, outmap, b));
        SSDCHK(upload_bn(h->wpool, b, cw));
    }
    return SSD_OK;
}

static int load_dw(ssd_handle *h, const std::string &scope, const std::string &bnname, int C, DwW &d, int in_split = 0)
{
    const Tensor *w = getvar(h, scope + "/depthwise_weights", {3, 3, C, 1});
    if (!w) return SSD_ERR_WEIGHT;
    d.Cp = in_split > 0 ? 2 * round_up(in_split, 32) : round_up(C, 32);
    std::vector<int> map = in_split > 0 ? twopart_map(in_split, round_up(in_split, 32)) : phys_map(C, d.Cp);
    BnHost b;
    SSDCHK(get_bn(h, scope + "/" + bnname, C, map, b));
    return upload_dw(h->wpool, permute_rows(w->data.data(), 9, C, map), b, d);
}

static int load_first(ssd_handle *h, const std::string &scope, const std::string &bnname, int Cout)
{
    const Tensor *w = getvar(h, scope + "/weights", {3, 3, 3, Cout});
    if (!w) return SSD_ERR_WEIGHT;
    const int Cp = round_up(Cout, 32);
    std::vector<int> map = phys_map(Cout, Cp);
    h->first.Cp = h->firstCp = Cp;
    BnHost b;
    SSDCHK(get_bn(h, scope + "/" + bnname, Cout, map, b));
    return upload_dw(h->wpool, permute_rows(w->data.data(), 27, Cout, map), b, h->first);
}

// mobilenet_v1.py:52-58
const int MB_STRIDE[13] = {1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1};
static const int MB_FILT[13] = {64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024};
static int mb_depth(int x, float dm) { int v = (int)(x * dm); return v > 8 ? v : 8; }

static int shuffle_initial_depth(float dm)
{
    // shufflenet_v2.py:22 `possibilities`, keyed by str(depth_multiplier) (model.py:29)
    if (dm == 0.5f) return 48;
    if (dm == 1.0f) return 116;
    if (dm == 1.5f) return 176;
    if (dm == 2.0f) return 224;
    return -1;
}

static int finalize_mobilenet(ssd_handle *h)
{
    const float dm = h->cfg.depth_multiplier;
    int c = mb_depth(32, dm);
    SSDCHK(load_first(h, "MobilenetV1/Conv2d_0", "BatchNorm", c));
    h->firstAct = SSD_ACT_RELU6;
    h->dw.resize(13);
    h->pw.resize(13);
    for (int i = 0; i < 13; ++i) {
        char s[96];
        snprintf(s, sizeof s, "MobilenetV1/Conv2d_%d_depthwise", i + 1);
        SSDCHK(load_dw(h, s, "BatchNorm", c, h->dw[i]));
        const int f = mb_depth(MB_FILT[i], dm);
        snprintf(s, sizeof s, "MobilenetV1/Conv2d_%d_pointwise", i + 1);
        SSDCHK(load_conv(h, std::string(s) + "/weights", std::string(s) + "/BatchNorm", 1, c, f, h->pw[i]));
        c = f;
        if (i == 4) h->c_ch[0] = c;
        if (i == 10) h->c_ch[1] = c;
        if (i == 12) h->c_ch[2] = c;
    }
    return SSD_OK;
}

// ShuffleNet layer order (execution order used by the plan, which finds each stage through h->sn_stage):
//   per stage: unit_1 {before, dw, after, second dw, second after}, units 2..n {before, dw, after}
//   then Conv5.
static int finalize_shufflenet(ssd_handle *h)
{
    const int D0 = shuffle_initial_depth(h->cfg.depth_multiplier);
    if (D0 < 0) return ssd_fail(SSD_ERR_INVALID, "shufflenet depth_multiplier must be 0.5, 1.0, 1.5 or 2.0");
    SSDCHK(load_first(h, "ShuffleNetV2/Conv1", "batch_norm", 24));
    h->firstAct = SSD_ACT_RELU;
    const int units[3] = {4, 8, 4};
    // A stage's output is kept in TWO-PART rows [x half | y half], each half (D channels) in its own standard layout over Dp
    // physical channels: the last unit's conv1x1_after then stores its channels as one dense run per position (plan.hip), and
    // the stage's consumers -- the next stage's unit_1 (conv1x1_before, second_branch depthwise + conv1x1_after), the FPN
    // lateral, Conv5 -- get their weights packed for that layout here.  Their k-ordered accumulation still visits the
    // logical channels in ascending order (the pad channels of the x half, zeros, sit between 2 D - 1's halves).
    int cin = 24, out = D0, split = 0;          // split: channels per half of this stage's input rows (0: standard rows)
    for (int st = 0; st < 3; ++st) {
        const int D = out / 2;
        h->sn_stage[st] = ssd_handle::SnStage{(int)h->pw.size(), (int)h->dw.size(), units[st]};
        char base[64];
        snprintf(base, sizeof base, "ShuffleNetV2/Stage%d", st + 2);
        std::string u1 = std::string(base) + "/unit_1";
        ConvW cw; DwW d;
        SSDCHK(load_conv(h, u1 + "/conv1x1_before/weights", u1 + "/conv1x1_before/batch_norm", 1, cin, cin, cw, false, split)); h->pw.push_back(cw);
        SSDCHK(load_dw(h, u1 + "/depthwise", "batch_norm", cin, d)); h->dw.push_back(d);
        cw = ConvW();
        SSDCHK(load_conv(h, u1 + "/conv1x1_after/weights", u1 + "/conv1x1_after/batch_norm", 1, cin, D, cw)); h->pw.push_back(cw);
        d = DwW();
        SSDCHK(load_dw(h, u1 + "/second_branch/depthwise", "batch_norm", cin, d, split)); h->dw.push_back(d);
        cw = ConvW();
        SSDCHK(load_conv(h, u1 + "/second_branch/conv1x1_after/weights", u1 + "/second_branch/conv1x1_after/batch_norm", 1, cin, D, cw, false, split)); h->pw.push_back(cw);
        for (int j = 2; j <= units[st]; ++j) {
            std::string u = std::string(base) + "/unit_" + std::to_string(j);
            cw = ConvW();
            SSDCHK(load_conv(h, u + "/conv1x1_before/weights", u + "/conv1x1_before/batch_norm", 1, D, D, cw)); h->pw.push_back(cw);
            // this layer exists ONLY as the gathering kernel (sn_pw.hip: concat_shuffle_split folded into its loads): a width that
            // kernel does not take must fail HERE, with the layer's name, not at the first forward (the size-dependent limits -- 2 GiB
            // per stage allocation -- are select_plans' sub-batch split)
            if (!pw_gather_supports(cw.CinP, cw.CoutP, 1, cw.CinP * 4, cw.CinP * 4, cw.CoutP * 4))
                return ssd_fail(SSD_ERR_INVALID, "ssd_finalize: " + u + "/conv1x1_before (" + std::to_string(D) + " -> " + std::to_string(D) +
                                                 " channels) is not a shape of the gathering 1x1 kernel (sn_pw.hip: 32 <= padded input channels <= 512)");
            d = DwW();
            SSDCHK(load_dw(h, u + "/depthwise", "batch_norm", D, d)); h->dw.push_back(d);
            cw = ConvW();
            SSDCHK(load_conv(h, u + "/conv1x1_after/weights", u + "/conv1x1_after/batch_norm", 1, D, D, cw)); h->pw.push_back(cw);
        }
        cin = out;
        split = D;
        if (st == 0) { h->c_ch[0] = out; h->c_split[0] = D; }
        if (st == 1) { h->c_ch[1] = out; h->c_split[1] = D; }
        out *= 2;
    }
    const int fin = h->cfg.depth_multiplier == 2.0f ? 2048 : 1024;
    ConvW cw;
    SSDCHK(load_conv(h, "ShuffleNetV2/Conv5/weights", "ShuffleNetV2/Conv5/batch_norm", 1, cin, fin, cw, false, split));
    h->pw.push_back(cw);
    h->c_ch[2] = fin;
    return SSD_OK;
}

static int finalize_fpn_heads(ssd_handle *h)
{
    // feature_extractor.py:55-74
    for (int i = 0; i < 3; ++i) {
        char n[48];
        snprintf(n, sizeof n, "fpn/lateral%d/kernel", i + 3);
        SSDCHK(load_conv(h, n, "", 1, h->c_ch[i], 256, h->lat[i], false, h->c_split[i]));
    }
    for (int i = 0; i < 5; ++i) {
        char n[48], b[48];
        snprintf(n, sizeof n, "fpn/p%d/kernel", i + 3);
        snprintf(b, sizeof b, "fpn/p%d_batch_norm", i + 3);
        SSDCHK(load_conv(h, n, b, 3, i == 3 ? h->c_ch[2] : 256, 256, h->pconv[i]));
    }
    {   // p3 | p4 | p5 | p7 again behind one pointer each (same shapes: 3x3, 256 -> 256, batch norm + ReLU): at batch 1 the
        // convolutions run as ONE launch whose levels carry their own kernel offset (plan.hip, IgemmLevel::wt_off) and
        // geometry (p7: stride 2, explicit pad)
        const int src_of[4] = {0, 1, 2, 4};
        ConvW &g = h->pgroup;
        g = h->pconv[0];
        g.wt16 = g.wt16w = nullptr;            // (exact fp32 only: the split-fp16 packs carry a per-convolution scale)
        const bool have_lat = h->pconv[0].wlat && h->pconv[1].wlat && h->pconv[2].wlat && h->pconv[4].wlat;
        g.wlat = nullptr;
        const size_t wn = (size_t)g.taps * g.CoutPad * g.CinP, pn = (size_t)g.CoutP;
        for (int i = 1; i < 4; ++i)
            if (h->pconv[src_of[i]].CoutPad != g.CoutPad || h->pconv[src_of[i]].CinP != g.CinP || h->pconv[src_of[i]].CoutP != g.CoutP)
                return ssd_fail(SSD_ERR_WEIGHT, "fpn p3 / p4 / p5 / p7 kernels differ in shape");
        SSDCHK(h->wpool.alloc((void **)&g.wt, 4 * wn * sizeof(float)));
        SSDCHK(h->wpool.alloc((void **)&g.mean, 4 * pn * sizeof(float)));
        SSDCHK(h->wpool.alloc((void **)&g.sf, 4 * pn * sizeof(float)));
        SSDCHK(h->wpool.alloc((void **)&g.beta, 4 * pn * sizeof(float)));
        if (have_lat) SSDCHK(h->wpool.alloc((void **)&g.wlat, 4 * wn * sizeof(float)));
        for (int i = 0; i < 4; ++i) {
            const ConvW &src = h->pconv[src_of[i]];
            if (have_lat) HIPCHK(hipMemcpy(g.wlat + i * wn, src.wlat, wn * sizeof(float), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(g.wt + i * wn, src.wt, wn * sizeof(float), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(g.mean + i * pn, src.mean, pn * sizeof(float), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(g.sf + i * pn, src.sf, pn * sizeof(float), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(g.beta + i * pn, src.beta, pn * sizeof(float), hipMemcpyDeviceToDevice));
        }
    }
    // box_predictor.py:107-155: conv weights shared across levels, batch norm per level
    const char *nets[2] = {"box_net", "class_net"};
    const int A = 6, C = h->cfg.num_classes;
    for (int t = 0; t < 2; ++t) {
        for (int i = 0; i < 4; ++i) {
            char n[64];
            snprintf(n, sizeof n, "%s/conv3x3_%d/kernel", nets[t], i);
            ConvW &cw = h->tower[t][i];
            SSDCHK(load_conv(h, n, "", 3, 256, 256, cw));
            BnHost b;
            std::vector<int> outmap = phys_map(256, 256);
            for (int l = 3; l <= 7; ++l) {
                char s[80];
                snprintf(s, sizeof s, "%s/batch_norm_%d_for_level_%d", nets[t], i, l);
                SSDCHK(get_bn(h, s, 256, outmap, b));
            }
            SSDCHK(upload_bn(h->wpool, b, cw));
        }
        const int Cout = t == 0 ? 4 * A : C * A;
        const std::string scope = std::string(nets[t]) + (t == 0 ? "/encoded_boxes" : "/logits");
        ConvW &cw = h->final_[t];
        const Tensor *bias = getvar(h, scope + "/bias", {Cout});
        if (!bias) return SSD_ERR_WEIGHT;
        SSDCHK(load_conv(h, scope + "/kernel", "", 3, 256, Cout, cw, /*out_identity=*/true, 0, t == 1 ? bias->data.data() : nullptr));
        std::vector<float> bpad(bias->data);
        bpad.resize((size_t)round_up(Cout, 4), 0.0f);     // the epilogue reads parameters 4 at a time
        SSDCHK(h->wpool.upload(&cw.bias, bpad));
    }
    return SSD_OK;
}

int finalize_weights(ssd_handle *h)
{
    int r = h->cfg.backbone == SSD_BACKBONE_MOBILENET ? finalize_mobilenet(h) : finalize_shufflenet(h);
    if (r == SSD_OK) r = finalize_fpn_heads(h);
    if (r != SSD_OK) {
        h->wpool.free_all();
        h->dw.clear(); h->pw.clear();
    }
    return r;
}
