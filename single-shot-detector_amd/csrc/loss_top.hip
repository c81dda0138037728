// The per-level top losses: of every (plane, image, level) segment of ssd_loss's per-anchor planes the ceil(n / 5) largest values in
// descending order, and their mean over the batch slot by slot (ssd.py:135-152, the ten `*_losses_on_level_*` histograms' input).
// Semantics, the count rule, the ORDER (the total order on bit patterns) and the mean's arithmetic: include/ssd_hip.h, block "the
// per-level top losses".
//
//   loss_top_select   one 1024-lane block per segment (p, b, l), the grid strides over the 2 * B * L segments.  Radix select, most
//                     significant digit first, four passes of 8 bits over the segment's keys: each pass counts the keys that share
//                     the prefix found so far into 256 LDS bins (integer atomics; a wave whose candidates all fall into ONE bin adds
//                     their number once -- a localisation plane is mostly +0.0 and would otherwise serialise every atomic on one
//                     address), then a suffix scan over the bins finds the digit that holds rank k.  After pass four the block
//                     knows T, the key of rank k, and g < k, the number of keys above T.  A fifth pass compacts the g keys above T
//                     into the LDS sort buffer (wave-aggregated append: arrival order is free, they are sorted next) and the slots
//                     [g, k) take T -- equal keys are equal values, so the tail of ties needs no sort.  A bitonic sort in
//                     descending order then runs over the next power of two of g only (slots [g, P) hold T, which lies below every
//                     key of [0, g)), and slots [0, k) go to V as floats.  The segment is read five times, four of them from L2, four
//                     16-byte loads per lane in flight; the sort reads eight pairs per lane before it writes the first.
//                     Loads: a row starts at any 4-byte address, so a scalar head runs up to the 16-byte boundary, 16-byte loads
//                     cover the body and a scalar tail the rest; no address outside the segment is read.
//   loss_top_mean     one lane per (p, l, j): the double sum over b ascending from +0.0, rounded once, one fp32 division.
// LDS is dynamic: the sort buffer (the next power of two of the call's largest k_l, at most SSD_LOSS_TOP_MAX_K keys = 128 KiB),
// then the 256 bins and the block's few scalars.  Integer LDS atomics only; no global atomics; reads the planes, writes V and means.
#include "train_table.h"

#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int LT_THREADS = 1024;                                    // loss_top_select: 16 waves, four per SIMD (a segment is ONE block's)
constexpr int LT_MEAN_THREADS = 256;
constexpr int LT_BINS = 256;
constexpr int LT_DEPTH = 4;                                         // 16-byte loads a lane issues before it uses the first
constexpr int LT_SORT_BATCH = 8;                                    // compare-exchanges a lane reads before it writes the first
constexpr int LT_TAIL_WORDS = LT_BINS + 8;                          // bins | wave totals [4] | digit, rank, count, spare
constexpr int LT_MAX_GRID = 2048;                                   // the metric family's cap: the rest is grid-strided
constexpr int64_t LT_MAX_N = (int64_t)1 << 24;                      // ceil(n / 5) is the reference's fp32 rule below this
static_assert((SSD_LOSS_TOP_MAX_K & (SSD_LOSS_TOP_MAX_K - 1)) == 0, "the cap is its own padded size");
static_assert((size_t)SSD_LOSS_TOP_MAX_K * 4 + LT_TAIL_WORDS * 4 <= 160 * 1024, "one workgroup's LDS on gfx950");

struct Levels {                                                     // by value: the kernel reads it from its argument segment
    int n[SSD_LOSS_MAX_LEVELS], off[SSD_LOSS_MAX_LEVELS], k[SSD_LOSS_MAX_LEVELS], koff[SSD_LOSS_MAX_LEVELS];
};

// a float's bits as an unsigned key whose integer order is the header's total order
__device__ __forceinline__ unsigned top_key(float x)
{
    const unsigned bits = __float_as_uint(x);
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float top_value(unsigned key) { return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu)); }

// f(key, valid) over the n floats at seg: every lane of the block calls f the same number of times (f may ballot); valid is false
// for a lane that holds no element in that call.
template <class F>
__device__ __forceinline__ void walk_segment(const gfloat *seg, int n, F f)
{
    const int tid = (int)threadIdx.x;
    const int to_boundary = (int)((4u - (unsigned)(((uintptr_t)seg >> 2) & 3)) & 3);
    const int head = to_boundary < n ? to_boundary : n;
    const int nq = (n - head) >> 2;
    {
        const bool in = tid < head;
        f(in ? top_key(seg[tid]) : 0u, in);
    }
    const gfloat *body = seg + head;
    for (int q0 = 0; q0 < nq; q0 += LT_DEPTH * LT_THREADS) {         // LT_DEPTH loads in flight per lane before the first f
        v4f x[LT_DEPTH];
#pragma unroll
        for (int u = 0; u < LT_DEPTH; ++u) {
            const int q = q0 + u * LT_THREADS + tid;
            x[u] = (v4f){0.f, 0.f, 0.f, 0.f};
            if (q < nq) x[u] = *(const gv4f *)(body + 4 * (int64_t)q);
        }
#pragma unroll
        for (int u = 0; u < LT_DEPTH; ++u) {
            const bool in = q0 + u * LT_THREADS + tid < nq;
#pragma unroll
            for (int e = 0; e < 4; ++e) f(top_key(x[u][e]), in);
        }
    }
    {
        const int start = head + 4 * nq;
        const bool in = tid < n - start;
        f(in ? top_key(seg[start + tid]) : 0u, in);
    }
}

// one count into the bins; a wave whose valid lanes all hold one bin adds their number once
__device__ __forceinline__ void bin_add(int *bins, int d, bool valid)
{
    const unsigned long long pending = __ballot(valid);
    if (pending == 0) return;                                        // uniform over the wave
    const int leader = __ffsll((long long)pending) - 1;
    const int ld = __builtin_amdgcn_readlane(d, leader);
    if (__ballot(valid && d != ld) == 0) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&bins[ld], __popcll(pending));
    } else if (valid) {
        atomicAdd(&bins[d], 1);
    }
}

__global__ __launch_bounds__(LT_THREADS) void loss_top_select(const float *__restrict__ cls_losses, const float *__restrict__ loc_losses,
                                                              int B, int N, int L, Levels lv, int K, int cap, float *__restrict__ V)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lt_lds[];
    unsigned *buf = lt_lds;                                          // [cap] keys
    int *bins = (int *)(lt_lds + cap);                               // [256]
    int *wsum = bins + LT_BINS;                                      // [4]
    int *sel = wsum + 4;                                             // digit, rank left inside it, the append counter
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segments = 2 * B * L;
    if (tid < LT_BINS) bins[tid] = 0;
    for (int s = (int)blockIdx.x; s < segments; s += (int)gridDim.x) {
        const int l = s % L, b = (s / L) % B, p = s / (L * B);
        const int n = lv.n[l], k = lv.k[l];
        const gfloat *seg = (const gfloat *)(p ? loc_losses : cls_losses) + (int64_t)b * N + lv.off[l];
        // ---- the key of rank k: four digits, most significant first
        unsigned prefix = 0;
        int rank = k;                                                // 1-based rank among the keys that share the prefix
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;
            __syncthreads();                                         // the bins are zero; sel was read
            walk_segment(seg, n, [&](unsigned key, bool in) {
                bin_add(bins, (int)((key >> shift) & 255u), in && (key & himask) == prefix); });
            __syncthreads();
            int h = 0, v = 0;
            if (tid < LT_BINS) {                                     // waves 0 .. 3, whole: one lane per bin
                h = bins[tid];
                bins[tid] = 0;
                v = h;                                               // the wave's inclusive suffix sum: digits tid .. 64 * wave + 63
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_down(v, d, 64);
                    if (lane + d < 64) v += t;
                }
                if (lane == 0) wsum[wave] = v;
            }
            __syncthreads();
            if (tid < LT_BINS) {
                int above_waves = 0;
                for (int w = wave + 1; w < LT_BINS / 64; ++w) above_waves += wsum[w];
                const int incl = v + above_waves, above = incl - h;  // keys of the prefix with digit >= tid, > tid
                if (above < rank && rank <= incl) {                  // exactly one lane: the prefix holds at least `rank` keys
                    sel[0] = tid;
                    sel[1] = rank - above;
                }
            }
            __syncthreads();
            prefix |= (unsigned)sel[0] << shift;
            rank = sel[1];
        }
        const unsigned T = prefix;
        const int g = k - rank;                                      // keys above T; `rank` slots take T
        // ---- the g keys above T, in arrival order
        if (tid == 0) sel[2] = 0;
        __syncthreads();
        walk_segment(seg, n, [&](unsigned key, bool in) {
            const bool take = in && key > T;
            const unsigned long long mask = __ballot(take);
            if (mask == 0) return;                                   // uniform over the wave
            const int leader = __ffsll((long long)mask) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&sel[2], __popcll(mask));
            base = __builtin_amdgcn_readlane(base, leader);
            const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (take && at < cap) buf[at] = key;                     // at < g < k <= cap by construction
        });
        int P = 1;
        while (P < g) P <<= 1;                                       // P <= the padded k <= cap
        const int filled = P > k ? P : k;
        for (int i = g + tid; i < filled; i += LT_THREADS) buf[i] = T;
        // ---- bitonic sort of [0, P), descending
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                // a stage's pairs are disjoint: a lane reads a batch of them, then writes it (the LDS latency is paid once a batch)
                for (int t0 = tid; t0 < (P >> 1); t0 += LT_SORT_BATCH * LT_THREADS) {
                    unsigned a[LT_SORT_BATCH], c[LT_SORT_BATCH];
#pragma unroll
                    for (int u = 0; u < LT_SORT_BATCH; ++u) {
                        const int t = t0 + u * LT_THREADS;
                        if (t < (P >> 1)) {
                            const int i = 2 * t - (t & (stride - 1));
                            a[u] = buf[i];
                            c[u] = buf[i + stride];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < LT_SORT_BATCH; ++u) {
                        const int t = t0 + u * LT_THREADS;
                        if (t < (P >> 1)) {
                            const int i = 2 * t - (t & (stride - 1));
                            const unsigned hi = max(a[u], c[u]), lo = min(a[u], c[u]);
                            const bool desc = (i & size) == 0;
                            buf[i] = desc ? hi : lo;
                            buf[i + stride] = desc ? lo : hi;
                        }
                    }
                }
            }
        __syncthreads();
        float *out = V + ((int64_t)p * B + b) * K + lv.koff[l];
        for (int i = tid; i < k; i += LT_THREADS) out[i] = top_value(buf[i]);
    }
}

__global__ __launch_bounds__(LT_MEAN_THREADS) void loss_top_mean(const float *__restrict__ V, int B, int K, float *__restrict__ means)
{
    const int total = 2 * K;
    const float fB = (float)B;
    for (int i = (int)blockIdx.x * LT_MEAN_THREADS + (int)threadIdx.x; i < total; i += (int)gridDim.x * LT_MEAN_THREADS) {
        const int p = i >= K ? 1 : 0, j = i - p * K;
        const float *col = V + (int64_t)p * B * K + j;
        double s = 0.0;
        for (int b = 0; b < B; ++b) s = s + (double)col[(int64_t)b * K];
        means[i] = __fdiv_rn((float)s, fB);
    }
}

std::atomic<unsigned> g_select_lds{0};

// the refusals every function of the family shares -> k_l, K and the largest k_l
int check_levels(const char *fn, const int64_t *anchors_per_level, int32_t n_levels, int64_t *k_out, int64_t *K_out, int64_t *N_out,
                 int64_t *kmax_out)
{
    const std::string name(fn);
    if (!anchors_per_level) return ssd_fail(SSD_ERR_INVALID, name + ": NULL anchors_per_level");
    if (n_levels < 1 || n_levels > SSD_LOSS_MAX_LEVELS)
        return ssd_fail(SSD_ERR_INVALID, name + ": n_levels must be in [1, " + std::to_string(SSD_LOSS_MAX_LEVELS) + "]");
    int64_t N = 0, K = 0, kmax = 0;
    for (int32_t l = 0; l < n_levels; ++l) {                         // the sizes first: no level of 2^24 anchors fits the cap below
        const int64_t n = anchors_per_level[l];
        if (n < 1) return ssd_fail(SSD_ERR_INVALID, name + ": anchors_per_level[" + std::to_string(l) + "] must be at least 1");
        if (n >= LT_MAX_N || N + n >= LT_MAX_N)
            return ssd_fail(SSD_ERR_INVALID, name + ": the levels' sum N must be below 2^24 (the count rule ceil(n / 5) is the reference's up to there)");
        N += n;
    }
    for (int32_t l = 0; l < n_levels; ++l) {
        const int64_t k = (anchors_per_level[l] + 4) / 5;
        if (k > SSD_LOSS_TOP_MAX_K)
            return ssd_fail(SSD_ERR_INVALID, name + ": level " + std::to_string(l) + " keeps " + std::to_string(k) + " values, above SSD_LOSS_TOP_MAX_K = " +
                                                 std::to_string(SSD_LOSS_TOP_MAX_K));
        if (k_out) k_out[l] = k;
        K += k;
        kmax = k > kmax ? k : kmax;
    }
    if (K_out) *K_out = K;
    if (N_out) *N_out = N;
    if (kmax_out) *kmax_out = kmax;
    return SSD_OK;
}

}  // namespace

extern "C" int64_t ssd_loss_top_counts(const int64_t *anchors_per_level, int32_t n_levels, int64_t *k_out)
{
    int64_t K = 0;
    if (!k_out) {
        ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_counts: NULL k_out");
        return -1;
    }
    if (check_levels("ssd_loss_top_counts", anchors_per_level, n_levels, k_out, &K, nullptr, nullptr) != SSD_OK) return -1;
    return K;
}

extern "C" size_t ssd_loss_top_workspace_bytes(int32_t B, const int64_t *anchors_per_level, int32_t n_levels)
{
    int64_t K = 0;
    if (B < 1) {
        ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_workspace_bytes: B must be at least 1");
        return 0;
    }
    if (check_levels("ssd_loss_top_workspace_bytes", anchors_per_level, n_levels, nullptr, &K, nullptr, nullptr) != SSD_OK) return 0;
    return (size_t)2 * (size_t)B * (size_t)K * sizeof(float);
}

extern "C" int ssd_loss_top_means(const float *cls_losses_dev, const float *loc_losses_dev, int32_t B, int32_t N, const int64_t *anchors_per_level,
                                  int32_t n_levels, float *means_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "ssd_loss_top_means";
    if (!cls_losses_dev || !loc_losses_dev || !means_dev) return ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_means: NULL cls_losses_dev, loc_losses_dev or means_dev");
    if (((uintptr_t)cls_losses_dev | (uintptr_t)loc_losses_dev | (uintptr_t)means_dev) & 3)
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_means: cls_losses_dev, loc_losses_dev and means_dev must be 4-byte aligned");
    if (B < 1) return ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_means: B must be at least 1");
    int64_t k[SSD_LOSS_MAX_LEVELS], K = 0, sum = 0, kmax = 0;
    SSDCHK(check_levels(fn, anchors_per_level, n_levels, k, &K, &sum, &kmax));
    if (sum != (int64_t)N)
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_means: the levels sum to " + std::to_string(sum) + " anchors, N is " + std::to_string(N));
    if (2 * (int64_t)B * n_levels > INT_MAX || (int64_t)B * N > ((int64_t)1 << 40))
        return ssd_fail(SSD_ERR_INVALID, "ssd_loss_top_means: B is too large");
    SSDCHK(check_workspace(fn, workspace, workspace_bytes, (size_t)2 * (size_t)B * (size_t)K * sizeof(float)));
    Levels lv = {};
    int off = 0, koff = 0;
    for (int32_t l = 0; l < n_levels; ++l) {
        lv.n[l] = (int)anchors_per_level[l];
        lv.off[l] = off;
        lv.k[l] = (int)k[l];
        lv.koff[l] = koff;
        off += lv.n[l];
        koff += lv.k[l];
    }
    int cap = 1;
    while (cap < kmax) cap <<= 1;                                    // <= SSD_LOSS_TOP_MAX_K
    const int lds_bytes = (cap + LT_TAIL_WORDS) * 4;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ssd_allow_lds((const void *)loss_top_select, (SSD_LOSS_TOP_MAX_K + LT_TAIL_WORDS) * 4, g_select_lds));
    const int64_t segments = 2 * (int64_t)B * n_levels;
    const unsigned grid = (unsigned)(segments < LT_MAX_GRID ? segments : LT_MAX_GRID);
    hipLaunchKernelGGL(loss_top_select, dim3(grid), dim3(LT_THREADS), (size_t)lds_bytes, s, cls_losses_dev, loc_losses_dev, (int)B, (int)N,
                       (int)n_levels, lv, (int)K, cap, (float *)workspace);
    HIPCHK(hipGetLastError());
    const int64_t mblocks = (2 * K + LT_MEAN_THREADS - 1) / LT_MEAN_THREADS;
    hipLaunchKernelGGL(loss_top_mean, dim3((unsigned)(mblocks < LT_MAX_GRID ? mblocks : LT_MAX_GRID)), dim3(LT_MEAN_THREADS), 0, s,
                       (const float *)workspace, (int)B, (int)K, means_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
