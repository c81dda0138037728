// The COCO accumulation: CocoBoxEval.accumulate() (coco_metric.py) for every (category, area range, maxDets) in one launch over
// ssd_coco_match's outputs.  Semantics, the layout and every refusal: include/ssd_hip.h, block "the COCO accumulation".
//
//   coco_accumulate   256 lanes per block, one wave per (k, a, m), SSD_COCO_CELLS_PER_BLOCK (4) of them per block; a grid of at most
//                     SSD_COCO_GRID_CAP blocks strides over the K * A * M items.  The waves of a block share nothing but the block's LDS,
//                     each its own 64 doubles: no __syncthreads, every wave makes its own number of passes.
//                     A wave first counts npig (ballots over the category's gt_ignore bytes) and forms c_r for r = lane and lane + 64:
//                     an estimate ceil(thr * npig) corrected by the exact test double(c) / double(npig) >= thr on its neighbours.
//                     Then two walks over the category's positions, 64 at a time: a coalesced load of `order`, gathered rank / matched /
//                     ignored words, and per threshold bit one ballot each of the true and the false positives.  What belongs to
//                     threshold t -- the totals, the running counts, the running suffix maximum -- lives in lane t and is read with
//                     v_readlane (t is the wave-uniform loop counter).
//                       forward    n and the totals tp, fp of all T thresholds from the same words;
//                       backward   from the last chunk to the first: the inclusive counts are the count in front of the chunk (the
//                                  running count minus the chunk's popcount) plus the popcount of the ballot's bits up to the lane;
//                                  pr_j by one correctly rounded division; the suffix maximum over the lanes in six shuffle steps,
//                                  then against the maximum of the chunks behind.  A row where tp steps to c puts its E at slot
//                                  c - 1 - (count in front of the chunk) of the wave's LDS row; the lanes of the r with c_r inside the
//                                  chunk's counts read their slot and store precision[t, r].
//                     What no row stores is stored once at the end: +0.0 for c_r > tp total (and for n == 0), E_0 -- the final running
//                     maximum -- for c_r == 0, and recall = tp total / npig.  Every element is written exactly once; no atomics.
#include "metric_host.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CA_THREADS = 256;
constexpr int CA_WAVES = SSD_COCO_CELLS_PER_BLOCK;
static_assert(CA_THREADS == 64 * CA_WAVES, "one wave per (k, a, m)");
static_assert(SSD_COCO_MAX_REC <= 128, "a lane owns the recall thresholds lane and lane + 64");
static_assert(SSD_COCO_MAX_THR <= 16, "the matching's words are uint16, bit t");
static_assert(sizeof(ssd_coco_segment) == 32 && offsetof(ssd_coco_segment, det_count) == 8 && offsetof(ssd_coco_segment, gt_begin) == 16 &&
              offsetof(ssd_coco_segment, gt_count) == 24, "ssd_coco_segment is the 32-byte row of include/ssd_hip.h");

struct AccParams {
    int max_dets[SSD_COCO_MAX_MAXDETS];
};

__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double lane_value(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// c_r of the header: the smallest integer c >= 0 with double(c) / double(npig) >= thr; 2^31, which no count reaches, when that is
// further than a count can go
__device__ __forceinline__ int64_t first_count(double thr, int64_t npig)
{
    if (!(thr > 0.0)) return 0;
    const double dn = (double)npig, cap = 2147483648.0;
    int64_t c = (int64_t)fmin(ceil(thr * dn), cap);
    while (c > 0 && (double)(c - 1) / dn >= thr) --c;
    while (c < (int64_t)cap && (double)c / dn < thr) ++c;
    return c;
}

__global__ __launch_bounds__(CA_THREADS) void coco_accumulate(const ssd_coco_segment *__restrict__ segments, int K,
                                                              const int32_t *__restrict__ order, const uint8_t *__restrict__ rank,
                                                              const uint16_t *__restrict__ matched, const uint16_t *__restrict__ ignored,
                                                              int64_t nd, const uint8_t *__restrict__ gt_ignore, int64_t ng, int T, int A, int M,
                                                              AccParams p, const double *__restrict__ rec_thr, int R,
                                                              double *__restrict__ precision, double *__restrict__ recall)
{
    __shared__ double s_e[CA_WAVES][64];

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    double *slot = s_e[wave];
    const unsigned long long upto = ~0ull >> (63 - lane);           // the lanes up to this one
    const double eps = 0x1p-52;
    const int64_t items = (int64_t)K * A * M, stride = (int64_t)gridDim.x * CA_WAVES;
    for (int64_t item = (int64_t)blockIdx.x * CA_WAVES + wave; item < items; item += stride) {
        const int m = (int)(item % M), a = (int)(item / M % A), k = (int)(item / ((int64_t)M * A));
        int maxdet = p.max_dets[0];
#pragma unroll
        for (int q = 1; q < SSD_COCO_MAX_MAXDETS; ++q) maxdet = m == q ? p.max_dets[q] : maxdet;
        const ssd_coco_segment seg = segments[k];
        const int64_t begin = seg.det_begin, count = seg.det_count;
        const uint16_t *__restrict__ mrow = matched + (int64_t)a * nd, *__restrict__ irow = ignored + (int64_t)a * nd;
        // recall[t, k, a, m] is element rec_at + t * rec_step, precision[t, r, k, a, m] element rec_at + (t * R + r) * pre_step
        const int64_t rec_at = ((int64_t)k * A + a) * M + m, rec_step = items, pre_step = items;

        // ---- npig: the zero bytes of the category's gt_ignore at this area range
        int64_t npig = 0;
        {
            const uint8_t *__restrict__ gi = gt_ignore + (int64_t)a * ng + seg.gt_begin;
            for (int64_t g0 = 0; g0 < seg.gt_count; g0 += 64) {
                const int64_t g = g0 + lane;
                npig += __popcll(__ballot(g < seg.gt_count && gi[g] == 0));
            }
        }
        if (npig == 0) {
            for (int i = lane; i < T * R; i += 64) precision[rec_at + (int64_t)i * pre_step] = -1.0;
            if (lane < T) recall[rec_at + (int64_t)lane * rec_step] = -1.0;
            continue;
        }
        const double dn = (double)npig;
        int64_t c[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = lane + 64 * q;
            c[q] = r < R ? first_count(rec_thr[r], npig) : INT64_MAX;
        }

        // one chunk of the category's positions: does the row take part, its matched / ignored words
        const auto load = [&](int64_t c0, bool &part, unsigned &tpw, unsigned &fpw) {
            const int64_t j = c0 + lane;
            const int64_t row = j < count ? (int64_t)order[begin + j] : -1;
            part = row >= 0 && row < nd && (int)rank[row] < maxdet;
            const unsigned mw = part ? mrow[row] : 0u, iw = part ? irow[row] : 0u;
            tpw = part ? (mw & ~iw) : 0u;                  // bit t: a true positive at threshold t
            fpw = part ? (~mw & ~iw) : 0u;                 // bit t: a false positive
        };

        // ---- forward: n and the totals; lane t keeps threshold t's
        int n = 0, tot_tp = 0, tot_fp = 0;
        for (int64_t c0 = 0; c0 < count; c0 += 64) {
            bool part;
            unsigned tpw, fpw;
            load(c0, part, tpw, fpw);
            n += __popcll(__ballot(part));
            for (int t = 0; t < T; ++t) {
                const int ntp = __popcll(__ballot((tpw >> t) & 1u)), nfp = __popcll(__ballot((fpw >> t) & 1u));
                tot_tp += lane == t ? ntp : 0;
                tot_fp += lane == t ? nfp : 0;
            }
        }

        // ---- backward: lane t keeps the counts through the end of the chunk and the maximum of the chunks behind it
        int run_tp = tot_tp, run_fp = tot_fp;
        double run_e = 0.0;                                 // pr is never below +0.0
        for (int64_t c0 = count > 0 ? (count - 1) / 64 * 64 : -64; c0 >= 0; c0 -= 64) {
            bool part;
            unsigned tpw, fpw;
            load(c0, part, tpw, fpw);
            for (int t = 0; t < T; ++t) {
                const bool is_tp = (tpw >> t) & 1u;
                const unsigned long long tpb = __ballot(is_tp), fpb = __ballot((fpw >> t) & 1u);
                const int end_tp = lane_value(run_tp, t), end_fp = lane_value(run_fp, t);
                const int front_tp = end_tp - __popcll(tpb), front_fp = end_fp - __popcll(fpb);
                const int tp = front_tp + __popcll(tpb & upto), fp = front_fp + __popcll(fpb & upto);
                const double pr = part ? (double)tp / (((double)fp + (double)tp) + eps) : 0.0;
                double e = pr;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const double o = __shfl_down(e, d, 64);
                    e = lane + d < 64 ? fmax(e, o) : e;
                }
                e = fmax(e, lane_value(run_e, t));
                const double head = lane_value(e, 0);
                if (lane == t) {
                    run_e = head;
                    run_tp = front_tp;
                    run_fp = front_fp;
                }
                wave_lds_sync();                            // the reads of the threshold before are done
                if (is_tp) slot[tp - front_tp - 1] = e;
                wave_lds_sync();
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int r = lane + 64 * q;
                    if (r < R && c[q] > front_tp && c[q] <= end_tp)
                        precision[rec_at + ((int64_t)t * R + r) * pre_step] = slot[(int)(c[q] - front_tp) - 1];
                }
            }
        }

        // ---- what no row stored
        for (int t = 0; t < T; ++t) {
            const int total = lane_value(tot_tp, t);
            const double e0 = lane_value(run_e, t);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = lane + 64 * q;
                if (r < R && (c[q] == 0 || c[q] > total))
                    precision[rec_at + ((int64_t)t * R + r) * pre_step] = c[q] == 0 && n > 0 ? e0 : 0.0;
            }
            if (lane == 0) recall[rec_at + (int64_t)t * rec_step] = (double)total / dn;
        }
    }
}

}  // namespace

extern "C" int ssd_coco_accumulate(const ssd_coco_segment *segments_host, const ssd_coco_segment *segments_dev, int32_t K,
                                   const int32_t *order_dev, const uint8_t *rank_dev, const uint16_t *matched_dev,
                                   const uint16_t *ignored_dev, int64_t nd, const uint8_t *gt_ignore_dev, int64_t ng, int32_t T, int32_t A,
                                   const int32_t *max_dets_host, int32_t M, const double *rec_thr_host, const double *rec_thr_dev, int32_t R,
                                   double *precision_dev, double *recall_dev, void *stream)
{
    const std::string who = "ssd_coco_accumulate";
    const auto range = [&](const char *name, int lo, int hi) {
        return ssd_fail(SSD_ERR_INVALID, who + ": " + name + " must be in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    };
    if (K < 0 || K > (1 << 20)) return ssd_fail(SSD_ERR_INVALID, who + ": K must be in [0, 2^20]");
    if (nd < 0 || nd > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": nd must be in [0, 2^31 - 1]");
    if (ng < 0 || ng > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": ng must be in [0, 2^40]");
    if (T < 1 || T > SSD_COCO_MAX_THR) return range("T", 1, SSD_COCO_MAX_THR);
    if (A < 1 || A > SSD_COCO_MAX_AREA) return range("A", 1, SSD_COCO_MAX_AREA);
    if (M < 1 || M > SSD_COCO_MAX_MAXDETS) return range("M", 1, SSD_COCO_MAX_MAXDETS);
    if (R < 1 || R > SSD_COCO_MAX_REC) return range("R", 1, SSD_COCO_MAX_REC);
    if (!max_dets_host) return ssd_fail(SSD_ERR_INVALID, who + ": max_dets_host is NULL");
    if (!rec_thr_host) return ssd_fail(SSD_ERR_INVALID, who + ": rec_thr_host is NULL");
    if (K > 0 && !segments_host) return ssd_fail(SSD_ERR_INVALID, who + ": segments_host is NULL");
    SSDCHK(check_ptrs(who, {{segments_dev, K > 0, 8, "segments_dev"}, {order_dev, nd > 0, 4, "order_dev"}, {rank_dev, nd > 0, 1, "rank_dev"},
                            {matched_dev, nd > 0, 2, "matched_dev"}, {ignored_dev, nd > 0, 2, "ignored_dev"},
                            {gt_ignore_dev, ng > 0, 1, "gt_ignore_dev"}, {rec_thr_dev, K > 0, 8, "rec_thr_dev"},
                            {precision_dev, K > 0, 8, "precision_dev"}, {recall_dev, K > 0, 8, "recall_dev"}}));
    for (int m = 0; m < M; ++m)
        if (max_dets_host[m] < 1 || (m > 0 && max_dets_host[m] <= max_dets_host[m - 1]))
            return ssd_fail(SSD_ERR_INVALID, who + ": max_dets_host[" + std::to_string(m) + "] must be positive and above the one before");
    for (int r = 0; r < R; ++r)
        if (!std::isfinite(rec_thr_host[r]) || (r > 0 && !(rec_thr_host[r] >= rec_thr_host[r - 1])))
            return ssd_fail(SSD_ERR_INVALID, who + ": rec_thr_host[" + std::to_string(r) + "] must be finite and not below the one before");
    const auto row = [&](int64_t k) { const ssd_coco_segment &x = segments_host[k]; return std::array<int64_t, 4>{x.det_begin, x.det_count, x.gt_begin, x.gt_count}; };
    int64_t det_end;
    SSDCHK(check_ranges(who, {"segment", "det_count", "gt_count", -1, -1, true}, K, nd, ng, row, &det_end));
    if (K > 0 && det_end != nd)
        return ssd_fail(SSD_ERR_INVALID, who + ": the segments' detection ranges end at " + std::to_string(det_end) + ", not at nd");
    if (K == 0) return SSD_OK;
    AccParams p;
    for (int m = 0; m < SSD_COCO_MAX_MAXDETS; ++m) p.max_dets[m] = max_dets_host[m < M ? m : 0];
    hipLaunchKernelGGL(coco_accumulate, dim3(wave_grid((int64_t)K * A * M)), dim3(CA_THREADS), 0, (hipStream_t)stream, segments_dev, (int)K, order_dev, rank_dev,
                       matched_dev, ignored_dev, nd, gt_ignore_dev, ng, (int)T, (int)A, (int)M, p, rec_thr_dev, (int)R, precision_dev,
                       recall_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
