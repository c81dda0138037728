// The TRAIN step's histograms: TF's default-bucket histogram (tf.summary.histogram) and its statistics of every variable and of
// every gradient of total_loss, over the update's table, before the update consumes the gradients.  Semantics, the limits, the
// bucket rule and the ORDER of the double additions: include/ssd_hip.h, block "the TRAIN step's histograms".
//
//   train_hist_clear    zeroes counts [T][2][NB] (the caller need not).
//   train_hist_blocks   stage 1 over the update's work list (train_table.h: the block shape, the row search, walk_block, whose
//                       tail path lets every lane visit all 16 positions: hist_add's ballots see the whole wave).
//                       Per element: the gradient plane's value g' (one fp32 multiply, one fp32 add), the two
//                       buckets, and per plane sum, sum of squares (double), min, max (as ordered integer keys), num and bad.  The
//                       bucket is the header's upper_bound: a guess from v_log_f32 corrected against the positive limits in LDS
//                       until the neighbouring limits bracket |x|, so that it equals the search on every float whatever the
//                       logarithm's error.  The block keeps a private histogram of both planes in LDS (integer atomics), flushes
//                       the non-zero buckets of the range it touched with vector global atomics and zeroes them again.  The
//                       doubles go through tree256; lane 0 writes the block's 64-byte partial.
//                       Contention: trained weights fall into a few dozen buckets and constant tensors (a fresh gamma, a zero
//                       gradient) into ONE, so the 64 lanes of an LDS atomic mostly hit a handful of addresses.  Equal buckets of a
//                       wave are aggregated before the atomic in the cheapest form that removes the worst case: the first valid
//                       lane's bucket is broadcast, and a wave whose valid lanes ALL hold it adds their number once (one ballot);
//                       any other wave takes the per-element atomic, whose same-address conflicts the LDS serialises at a cost
//                       measured as 1.5 x at the very worst.  Option "hist_scheme" picks the form: 0 the naive one (an atomic per
//                       element), 1 this one, 2 / 3 one / two full rounds (the lanes sharing the first pending lane's bucket are
//                       counted and added by one lane, the rest goes on), 4 rounds until nothing is pending -- counts are integers,
//                       every scheme gives the same bits; DESIGN.md 4.18 has what each measured.
//   train_hist_rows     stage 2: one wave per tensor adds its blocks' partials in ascending block order (wave_ordered_add).
// Integer atomics only; reads w and grad, writes the workspace and the outputs only.
#include "train_table.h"

#include <cfloat>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int HST_MAX_HALF = 800;                                   // LDS room for the positive limits (the loop gives 775)
constexpr int HST_MAX_NB = 2 * HST_MAX_HALF + 1;
constexpr int HST_UNIFORM = -1;                                     // hist_add's one-ballot form
constexpr int HST_PEEL_ALL = 64;
constexpr int HST_SCHEME_DEFAULT = 1;                               // option "hist_scheme" when unset (DESIGN.md 4.18 has the measurement)
static_assert(sizeof(ssd_histogram_stats) == SSD_HISTOGRAM_STATS_BYTES, "ssd_histogram_stats is 40 bytes, no padding");

constexpr unsigned KEY_POS_INF = 0xff800000u;                       // key(+inf): above every finite key
constexpr unsigned KEY_NEG_INF = 0x007fffffu;                       // key(-inf): below every finite key

struct Plane {                                                      // one lane's, one block's, one row's statistics of a plane
    double sum, sq;
    unsigned kmin, kmax;                                            // ordered keys: -FLT_MAX < ... < -0.0 < +0.0 < ... < FLT_MAX
    int num, bad;
};

struct Partial {                                                    // SSD_HISTOGRAM_BLOCK_BYTES: one block's result
    double sw, qw, sg, qg;
    unsigned kminw, kmaxw, kming, kmaxg;
    int numw, badw, numg, badg;
};
static_assert(sizeof(Partial) == SSD_HISTOGRAM_BLOCK_BYTES, "a partial is four doubles and eight 32-bit words");

// the limits of the header, built by its loop: the ONE definition (ssd_histogram_limits, the tests' helper compares against it,
// the caller uploads it)
const std::vector<double> &limits_table()
{
    static const std::vector<double> table = [] {
        std::vector<double> pos;
        double v = 1e-12;
        while (v < 1e20) {
            pos.push_back(v);
            v *= 1.1;
        }
        pos.push_back(DBL_MAX);
        std::vector<double> all;
        for (size_t i = pos.size(); i-- > 0;) all.push_back(-pos[i]);
        all.push_back(0.0);
        all.insert(all.end(), pos.begin(), pos.end());
        return all;
    }();
    return table;
}

// a float's bits as an unsigned key whose integer order is the order of the values, with -0.0 below +0.0
__device__ __forceinline__ unsigned order_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float key_value(unsigned key) { return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu)); }

// The bucket of a finite x: the number of limits <= (double)x.  With P the M positive limits (P[M - 1] = DBL_MAX, above every float):
//   x >= 0 (both zeros):  M + 1 + #{k: P[k] <= x}          x < 0:  M - #{k: P[k] < -x}
// Either count is the first index g whose limit is "above" |x| (x >= 0: P[g] > |x|; x < 0: P[g] >= |x|): both signs walk the same
// loops with their own comparison, so a wave of mixed signs does not run them twice.  g starts at floor(log1.1(|x| / 1e-12)) + 1
// from the hardware logarithm -- the answer itself unless the logarithm's error crosses a limit -- and moves until P[g - 1] is not
// above and P[g] is, so the result is the search's whatever the guess was.
__device__ __forceinline__ int bucket_of(float x, const double *P, int M)
{
    const unsigned bits = __float_as_uint(x);
    const bool neg = (bits >> 31) != 0 && (bits & 0x7fffffffu) != 0;
    const float ax = __uint_as_float(bits & 0x7fffffffu);
    const double d = (double)ax;
    float gf = (__log2f(ax) + 39.863137f) * 7.2725409f;             // log2(1e12), 1 / log2(1.1)
    gf = fminf(fmaxf(gf + 1.0f, 0.0f), (float)(M - 1));             // -inf (zero, a flushed denormal) and NaN end at 0
    int g = (int)gf;
    const auto above = [&](double p) { return neg ? p >= d : p > d; };
    while (g > 0 && above(P[g - 1])) --g;
    while (g < M - 1 && !above(P[g])) ++g;
    return neg ? M - g : M + 1 + g;
}

// one count into the block's LDS histogram.  PEEL > 0: that many rounds of wave aggregation, then the per-element atomic for what is
// left; PEEL == HST_UNIFORM: one ballot -- a wave whose valid lanes all hold one bucket adds their number once, any other wave takes
// the per-element atomic; PEEL == 0: the per-element atomic alone.
template <int PEEL>
__device__ __forceinline__ void hist_add(int *hist, int b, bool valid)
{
    bool todo = valid;
    if (PEEL == HST_UNIFORM) {
        const unsigned long long pending = __ballot(valid);
        if (pending != 0) {                                          // uniform over the lanes that are here
            const int leader = __ffsll((long long)pending) - 1;
            const int lb = __builtin_amdgcn_readlane(b, leader);
            if (__ballot(valid && b != lb) == 0) {
                if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], __popcll(pending));
                todo = false;
            }
        }
    } else if (PEEL > 0) {
        const int lane = (int)(threadIdx.x & 63);
#pragma unroll 1
        for (int i = 0; i < PEEL; ++i) {
            const unsigned long long pending = __ballot(todo);
            if (pending == 0) break;                                 // uniform over the lanes that are here
            const int leader = __ffsll((long long)pending) - 1;
            const int lb = __builtin_amdgcn_readlane(b, leader);
            const bool same = todo && b == lb;
            const unsigned long long mates = __ballot(same);
            if (lane == leader) atomicAdd(&hist[lb], __popcll(mates));
            todo = todo && !same;
        }
    }
    if (todo) atomicAdd(&hist[b], 1);
}

// one element of the tensor: x of w, g of grad -> both planes
template <bool GRAD, int PEEL>
__device__ __forceinline__ void hist_one(float x, float g, bool in, bool decay, float weight_decay, const double *P, int M, int *hist,
                                         int NBpad, Plane &pw, Plane &pg, int &blo, int &bhi)
{
    {
        const unsigned bits = __float_as_uint(x);
        const bool finite = in && (bits & 0x7f800000u) != 0x7f800000u;
        const double d = (double)x;
        pw.sum = pw.sum + (finite ? d : 0.0);
        pw.sq = pw.sq + (finite ? d * d : 0.0);
        const unsigned key = order_key(bits);
        pw.kmin = finite ? min(pw.kmin, key) : pw.kmin;
        pw.kmax = finite ? max(pw.kmax, key) : pw.kmax;
        pw.num += finite ? 1 : 0;
        pw.bad += (in && !finite) ? 1 : 0;
        const int b = finite ? bucket_of(x, P, M) : M;
        blo = finite ? min(blo, b) : blo;
        bhi = finite ? max(bhi, b) : bhi;
        hist_add<PEEL>(hist, b, finite);
    }
    if (GRAD) {
        const float prod = weight_decay * x;
        const float gp = decay ? g + prod : g;
        const unsigned bits = __float_as_uint(gp);
        const bool finite = in && (bits & 0x7f800000u) != 0x7f800000u;
        const double d = (double)gp;
        pg.sum = pg.sum + (finite ? d : 0.0);
        pg.sq = pg.sq + (finite ? d * d : 0.0);
        const unsigned key = order_key(bits);
        pg.kmin = finite ? min(pg.kmin, key) : pg.kmin;
        pg.kmax = finite ? max(pg.kmax, key) : pg.kmax;
        pg.num += finite ? 1 : 0;
        pg.bad += (in && !finite) ? 1 : 0;
        const int b = finite ? bucket_of(gp, P, M) : M;
        blo = finite ? min(blo, b) : blo;
        bhi = finite ? max(bhi, b) : bhi;
        hist_add<PEEL>(hist + NBpad, b, finite);
    }
}

__global__ __launch_bounds__(TBL_THREADS) void train_hist_clear(unsigned long long *__restrict__ counts, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * TBL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TBL_THREADS) counts[i] = 0;
}

template <int PEEL>
__global__ __launch_bounds__(TBL_THREADS) void train_hist_blocks(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                                 float weight_decay, const double *__restrict__ limits, int NB,
                                                                 unsigned long long *__restrict__ counts, Partial *__restrict__ partials)
{
    __shared__ double lds_p[HST_MAX_HALF];                           // the positive limits
    __shared__ int lds_hist[2 * HST_MAX_NB];                         // the block's histogram of both planes
    __shared__ double lds_d[4][TBL_THREADS];
    __shared__ unsigned lds_u[4][TBL_THREADS];
    __shared__ int lds_i[4][TBL_THREADS];
    __shared__ int lds_range[2];
    const int tid = (int)threadIdx.x;
    const int M = (NB - 1) >> 1;
    for (int i = tid; i < M; i += TBL_THREADS) lds_p[i] = limits[M + 1 + i];
    for (int i = tid; i < 2 * HST_MAX_NB; i += TBL_THREADS) lds_hist[i] = 0;
    __syncthreads();
    for (int c = (int)blockIdx.x; c < total_blocks; c += (int)gridDim.x) {
        const int row = row_of_block(tensors, T, &ssd_update_tensor::first_block, c);
        const ssd_update_tensor r = tensors[row];
        const gfloat *w = (const gfloat *)r.w, *grad = (const gfloat *)r.grad;
        const int pad = (int)(((uintptr_t)w & 15) >> 2);
        const bool gvec = (((uintptr_t)grad ^ (uintptr_t)w) & 15) == 0;
        const int64_t j0 = (int64_t)(c - r.first_block) * SSD_UPDATE_BLOCK_ELEMS;
        Plane pw = {0.0, 0.0, KEY_POS_INF, KEY_NEG_INF, 0, 0}, pg = pw;
        int blo = NB, bhi = -1;
        const bool decay = r.decay != 0;
        if (grad) walk_block<true>(w, grad, r.count, j0, pad, gvec, [&](float x, float g, bool in) {
            hist_one<true, PEEL>(x, g, in, decay, weight_decay, lds_p, M, lds_hist, HST_MAX_NB, pw, pg, blo, bhi); });
        else walk_block<false>(w, grad, r.count, j0, pad, false, [&](float x, float g, bool in) {
            hist_one<false, PEEL>(x, g, in, false, weight_decay, lds_p, M, lds_hist, HST_MAX_NB, pw, pg, blo, bhi); });
        // the four doubles go through tree256; the keys, the counts and the bucket range are integers (any order): a lane holds at
        // most 16 elements of each kind and a block 4096, so num and bad of a plane travel in one int
        lds_u[0][tid] = pw.kmin;
        lds_u[1][tid] = pw.kmax;
        lds_u[2][tid] = pg.kmin;
        lds_u[3][tid] = pg.kmax;
        lds_i[0][tid] = pw.num | (pw.bad << 16);
        lds_i[1][tid] = pg.num | (pg.bad << 16);
        lds_i[2][tid] = blo;
        lds_i[3][tid] = bhi;
        double d[4] = {pw.sum, pw.sq, pg.sum, pg.sq};
        tree256<4>(d, lds_d);
        if (tid < 64) {
            unsigned u[4];
            int n[2], rlo, rhi;
            u[0] = min(min(lds_u[0][tid], lds_u[0][tid + 128]), min(lds_u[0][tid + 64], lds_u[0][tid + 192]));
            u[1] = max(max(lds_u[1][tid], lds_u[1][tid + 128]), max(lds_u[1][tid + 64], lds_u[1][tid + 192]));
            u[2] = min(min(lds_u[2][tid], lds_u[2][tid + 128]), min(lds_u[2][tid + 64], lds_u[2][tid + 192]));
            u[3] = max(max(lds_u[3][tid], lds_u[3][tid + 128]), max(lds_u[3][tid + 64], lds_u[3][tid + 192]));
            n[0] = lds_i[0][tid] + lds_i[0][tid + 128] + lds_i[0][tid + 64] + lds_i[0][tid + 192];
            n[1] = lds_i[1][tid] + lds_i[1][tid + 128] + lds_i[1][tid + 64] + lds_i[1][tid + 192];
            rlo = min(min(lds_i[2][tid], lds_i[2][tid + 128]), min(lds_i[2][tid + 64], lds_i[2][tid + 192]));
            rhi = max(max(lds_i[3][tid], lds_i[3][tid + 128]), max(lds_i[3][tid + 64], lds_i[3][tid + 192]));
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                u[0] = min(u[0], (unsigned)__shfl_down((int)u[0], s, 64));
                u[1] = max(u[1], (unsigned)__shfl_down((int)u[1], s, 64));
                u[2] = min(u[2], (unsigned)__shfl_down((int)u[2], s, 64));
                u[3] = max(u[3], (unsigned)__shfl_down((int)u[3], s, 64));
                n[0] += __shfl_down(n[0], s, 64);
                n[1] += __shfl_down(n[1], s, 64);
                rlo = min(rlo, __shfl_down(rlo, s, 64));
                rhi = max(rhi, __shfl_down(rhi, s, 64));
            }
            if (tid == 0) {
                Partial p;
                p.sw = d[0];
                p.qw = d[1];
                p.sg = d[2];
                p.qg = d[3];
                p.kminw = u[0];
                p.kmaxw = u[1];
                p.kming = u[2];
                p.kmaxg = u[3];
                p.numw = n[0] & 0xffff;
                p.badw = n[0] >> 16;
                p.numg = n[1] & 0xffff;
                p.badg = n[1] >> 16;
                partials[c] = p;
                lds_range[0] = rlo;
                lds_range[1] = rhi;
            }
        }
        __syncthreads();                                             // the range; every LDS atomic of the block has landed
        // the flush: the non-zero buckets of the touched range of both planes, and the block's histogram is zero again
        const int rlo = lds_range[0], width = lds_range[1] - rlo + 1;
        unsigned long long *out = counts + (int64_t)row * 2 * NB;
        for (int i = tid; i < 2 * width; i += TBL_THREADS) {
            const int plane = i >= width ? 1 : 0;
            const int b = rlo + (i - plane * width);
            const int v = lds_hist[plane * HST_MAX_NB + b];
            if (v != 0) {
                atomicAdd(out + plane * NB + b, (unsigned long long)v);
                lds_hist[plane * HST_MAX_NB + b] = 0;
            }
        }
        __syncthreads();                                             // the next block of the stride writes the LDS again
    }
}

// stage 2, one wave per tensor.  Keys and counts are integers: each lane keeps its own and the wave combines them at the end.
__global__ __launch_bounds__(TBL_WAVE) void train_hist_rows(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                            const Partial *__restrict__ partials, ssd_histogram_stats *__restrict__ stats)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = tensors[t].first_block;
    const int last = t + 1 < T ? tensors[t + 1].first_block : total_blocks;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned kminw = KEY_POS_INF, kmaxw = KEY_NEG_INF, kming = KEY_POS_INF, kmaxg = KEY_NEG_INF;
    long long numw = 0, badw = 0, numg = 0, badg = 0;
    for (int base = first; base < last; base += TBL_WAVE) {
        Partial p = {0.0, 0.0, 0.0, 0.0, KEY_POS_INF, KEY_NEG_INF, KEY_POS_INF, KEY_NEG_INF, 0, 0, 0, 0};
        if (base + lane < last) p = partials[base + lane];
        kminw = min(kminw, p.kminw);
        kmaxw = max(kmaxw, p.kmaxw);
        kming = min(kming, p.kming);
        kmaxg = max(kmaxg, p.kmaxg);
        numw += p.numw;
        badw += p.badw;
        numg += p.numg;
        badg += p.badg;
        const double v[4] = {p.sw, p.qw, p.sg, p.qg};
        wave_ordered_add<4>(s, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        kminw = min(kminw, (unsigned)__shfl_xor((int)kminw, m, 64));
        kmaxw = max(kmaxw, (unsigned)__shfl_xor((int)kmaxw, m, 64));
        kming = min(kming, (unsigned)__shfl_xor((int)kming, m, 64));
        kmaxg = max(kmaxg, (unsigned)__shfl_xor((int)kmaxg, m, 64));
        numw += __shfl_xor(numw, m, 64);
        badw += __shfl_xor(badw, m, 64);
        numg += __shfl_xor(numg, m, 64);
        badg += __shfl_xor(badg, m, 64);
    }
    if (lane == 0) {
        ssd_histogram_stats a, b;
        a.sum = s[0];
        a.sum_squares = s[1];
        a.min = key_value(kminw);
        a.max = key_value(kmaxw);
        a.num = numw;
        a.bad = badw;
        b.sum = s[2];
        b.sum_squares = s[3];
        b.min = key_value(kming);
        b.max = key_value(kmaxg);
        b.num = numg;
        b.bad = badg;
        stats[2 * t] = a;
        stats[2 * t + 1] = b;
    }
}

template <int PEEL>
void launch_blocks(unsigned grid, hipStream_t stream, const ssd_update_tensor *tensors_dev, int T, int blocks, float weight_decay,
                   const double *limits_dev, int NB, unsigned long long *counts, Partial *partials)
{
    hipLaunchKernelGGL(train_hist_blocks<PEEL>, dim3(grid), dim3(TBL_THREADS), 0, stream, tensors_dev, T, blocks, weight_decay, limits_dev, NB,
                       counts, partials);
}

}  // namespace

extern "C" int32_t ssd_histogram_limits(double *out, int32_t capacity)
{
    const std::vector<double> &table = limits_table();
    const int32_t NB = (int32_t)table.size();
    if (out && capacity >= NB)
        for (int32_t i = 0; i < NB; ++i) out[i] = table[(size_t)i];
    return NB;
}

extern "C" size_t ssd_train_histograms_workspace_bytes(const ssd_update_tensor *tensors_host, int32_t T)
{
    return update_table_bytes("ssd_train_histograms_workspace_bytes", tensors_host, T, SSD_HISTOGRAM_BLOCK_BYTES);
}

extern "C" int ssd_train_histograms(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, float weight_decay,
                                    const double *limits_dev, int64_t *counts, ssd_histogram_stats *stats, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    int64_t blocks = 0;
    SSDCHK(check_update_table("ssd_train_histograms", tensors_host, tensors_dev, T, &blocks));
    if (!std::isfinite(weight_decay)) return ssd_fail(SSD_ERR_INVALID, "ssd_train_histograms: weight_decay is not finite");
    if (!limits_dev || !counts || !stats) return ssd_fail(SSD_ERR_INVALID, "ssd_train_histograms: NULL limits_dev, counts or stats");
    if (((uintptr_t)limits_dev | (uintptr_t)counts | (uintptr_t)stats) & 7)
        return ssd_fail(SSD_ERR_INVALID, "ssd_train_histograms: limits_dev, counts and stats must be 8-byte aligned");
    SSDCHK(check_workspace("ssd_train_histograms", workspace, workspace_bytes, (size_t)blocks * SSD_HISTOGRAM_BLOCK_BYTES));
    const int NB = (int)limits_table().size();
    if (NB > HST_MAX_NB) return ssd_fail(SSD_ERR_INVALID, "ssd_train_histograms: the limits table outgrew the kernel's LDS room");
    const int scheme = ssd_opt(nullptr, OPT_HIST_SCHEME, -1);
    const int pick = scheme < 0 ? HST_SCHEME_DEFAULT : scheme;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = (int64_t)T * 2 * NB;
    const unsigned cgrid = grid_for((cells + TBL_THREADS - 1) / TBL_THREADS);
    hipLaunchKernelGGL(train_hist_clear, dim3(cgrid), dim3(TBL_THREADS), 0, s, (unsigned long long *)counts, cells);
    HIPCHK(hipGetLastError());
    if (blocks > 0) {
        const unsigned grid = grid_for(blocks);
        unsigned long long *c = (unsigned long long *)counts;
        Partial *p = (Partial *)workspace;
        if (pick == 0) launch_blocks<0>(grid, s, tensors_dev, (int)T, (int)blocks, weight_decay, limits_dev, NB, c, p);
        else if (pick == 1) launch_blocks<HST_UNIFORM>(grid, s, tensors_dev, (int)T, (int)blocks, weight_decay, limits_dev, NB, c, p);
        else if (pick == 2) launch_blocks<1>(grid, s, tensors_dev, (int)T, (int)blocks, weight_decay, limits_dev, NB, c, p);
        else if (pick == 3) launch_blocks<2>(grid, s, tensors_dev, (int)T, (int)blocks, weight_decay, limits_dev, NB, c, p);
        else launch_blocks<HST_PEEL_ALL>(grid, s, tensors_dev, (int)T, (int)blocks, weight_decay, limits_dev, NB, c, p);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(train_hist_rows, dim3((unsigned)T), dim3(TBL_WAVE), 0, s, tensors_dev, (int)T, (int)blocks,
                       (const Partial *)workspace, stats);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
