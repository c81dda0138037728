// The VOC-style metric: coco_eval.Evaluator.evaluate() in two launches.  Semantics, the packed layout and every refusal:
// include/ssd_hip.h, block "the VOC-style metric".
//
//   voc_match   256 lanes per block, one wave per (label, image) cell, SSD_VOC_CELLS_PER_BLOCK (4) cells per block; a grid of at most
//               SSD_VOC_GRID_CAP blocks strides over the cell list.  The waves of a block share nothing: no LDS, no barrier.  The
//               loop over the cell's detections is wave-uniform (the cell row and the detection's box are scalar loads); lane l
//               forms IoU(d, g) for g = l + 64 * j in ascending j and keeps its first maximum under a strict >.  Every lane forms an
//               IoU from the same words with the same operations, so the wave's maximum (fmax over six cross-lane steps: exact, the
//               values are never NaN) is the bit pattern some lane holds, and the smallest g among the lanes that hold it is the
//               first maximum of the cell.  The lane g & 63 owns box g: bit g >> 6 of its 64-bit `taken` mask; one ballot tells the
//               wave whether the chosen box was taken.  Lane 0 stores tp and tp_iou at the detection's pos.
//   voc_curve   the same shape, one wave per label.  64 rows at a time (the next 64 are loaded before this chunk's chain of
//               additions starts): the inclusive count of true positives is a running carry plus the popcount of the ballot's bits
//               up to the lane -- integers; P, R and the score to maximise are formed per lane, each lane keeps its first maximum
//               (its rows ascend), and the final reduction takes the larger score and of equal scores the smaller row.  The terms
//               of ap and iou_sum go through wave_ordered_add<2> (train_table.h): dependent additions in ascending lane order,
//               which is ascending row order; a lane past the end adds +0.0 to sums that are never -0.0.
#include "metric_host.h"
#include "train_table.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int VM_THREADS = 256;
constexpr int VM_WAVES = SSD_VOC_CELLS_PER_BLOCK;
static_assert(VM_THREADS == 64 * VM_WAVES, "one wave per cell / label");
static_assert(SSD_VOC_MAX_GT == 64 * 64, "a lane keeps one 64-bit taken mask for the boxes lane + 64 * j");
static_assert(sizeof(ssd_voc_cell) == 24 && offsetof(ssd_voc_cell, gt_begin) == 8 && offsetof(ssd_voc_cell, D) == 16 &&
              offsetof(ssd_voc_cell, G) == 20, "ssd_voc_cell is the 24-byte row of include/ssd_hip.h");
static_assert(sizeof(ssd_voc_segment) == 24, "ssd_voc_segment is the 24-byte row of include/ssd_hip.h");
static_assert(sizeof(ssd_voc_result) == 64 && offsetof(ssd_voc_result, tp) == 40, "ssd_voc_result is the 64-byte row of include/ssd_hip.h");

// _iou_matrix of coco_eval.py on one pair of (ymin, xmin, ymax, xmax) boxes: every operation rounded once
__device__ __forceinline__ double iou_yxyx(double dy0, double dx0, double dy1, double dx1, double a_d, const double *__restrict__ g)
{
    const double gy0 = g[0], gx0 = g[1], gy1 = g[2], gx1 = g[3];
    const double w = fmin(dx1, gx1) - fmax(dx0, gx0);
    const double h = fmin(dy1, gy1) - fmax(dy0, gy0);
    const double inter = (w > 0.0 && h > 0.0) ? w * h : 0.0;
    if (!(inter > 0.0)) return 0.0;
    const double a_g = (gx1 - gx0) * (gy1 - gy0);
    return inter / ((a_d + a_g) - inter);
}

__global__ __launch_bounds__(VM_THREADS) void voc_match(const ssd_voc_cell *__restrict__ cells, int64_t n_cells,
                                                        const double *__restrict__ det_box, const int32_t *__restrict__ det_pos,
                                                        const double *__restrict__ gt_box, double thr, uint8_t *__restrict__ tp,
                                                        double *__restrict__ tp_iou, int64_t n_rows)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * VM_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * VM_WAVES + wave; c < n_cells; c += stride) {
        const ssd_voc_cell cell = cells[c];
        const int D = cell.D, G = cell.G;
        const double *__restrict__ gb = gt_box + cell.gt_begin * 4;
        unsigned long long taken = 0ull;                // bit j: box lane + 64 * j
        for (int d = 0; d < D; ++d) {
            const double *__restrict__ db = det_box + (cell.det_begin + d) * 4;
            const double dy0 = db[0], dx0 = db[1], dy1 = db[2], dx1 = db[3];
            const double a_d = (dx1 - dx0) * (dy1 - dy0);
            double best = -1.0;                         // below every IoU: a lane without a box never holds the maximum of a cell with boxes
            int best_g = INT_MAX;
            for (int g = lane; g < G; g += 64) {
                const double iou = iou_yxyx(dy0, dx0, dy1, dx1, a_d, gb + (int64_t)g * 4);
                if (iou > best) {
                    best = iou;
                    best_g = g;
                }
            }
            double top = best;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) top = fmax(top, __shfl_xor(top, m, 64));
            int first = best == top ? best_g : INT_MAX;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) first = min(first, __shfl_xor(first, m, 64));
            const bool good = top > 0.0 && top >= thr;  // wave-uniform; implies G > 0 and first < G
            const bool mine = good && (first & 63) == lane;
            const bool was = mine && ((taken >> (first >> 6)) & 1ull);
            const bool hit = good && __ballot(was) == 0ull;
            if (mine && hit) taken |= 1ull << (first >> 6);
            if (lane == 0) {
                const int64_t pos = det_pos[cell.det_begin + d];
                if (pos >= 0 && pos < n_rows) {
                    tp[pos] = hit ? 1 : 0;
                    tp_iou[pos] = hit ? top : 0.0;
                }
            }
        }
    }
}

__global__ __launch_bounds__(VM_THREADS) void voc_curve(const ssd_voc_segment *__restrict__ segments, int n_labels,
                                                        const uint8_t *__restrict__ tp, const double *__restrict__ tp_iou,
                                                        const double *__restrict__ conf, ssd_voc_result *__restrict__ results)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int stride = (int)gridDim.x * VM_WAVES;
    for (int l = (int)blockIdx.x * VM_WAVES + wave; l < n_labels; l += stride) {
        const ssd_voc_segment seg = segments[l];
        const int64_t begin = seg.begin, n = seg.count;
        const double num_gt = (double)seg.num_gt;
        int64_t carry = 0;                              // true positives of the chunks before
        double sums[2] = {0.0, 0.0};                    // ap, iou_sum
        double top = -INFINITY, top_p = 0.0, top_r = 0.0;
        int64_t top_k = INT64_MAX;
        bool t_next = lane < n && tp[begin + lane] != 0;
        double u_next = lane < n ? tp_iou[begin + lane] : 0.0;
        for (int64_t k0 = 0; k0 < n; k0 += 64) {
            const int64_t k = k0 + lane;
            const bool in = k < n, t = t_next;
            const double u = u_next;
            t_next = k + 64 < n && tp[begin + k + 64] != 0;
            u_next = k + 64 < n ? tp_iou[begin + k + 64] : 0.0;
            const unsigned long long hits = __ballot(t);
            const int64_t ctp = carry + __popcll(hits & (~0ull >> (63 - lane)));
            carry += __popcll(hits);
            const double P = (double)ctp / (double)(k + 1), R = (double)ctp / num_gt;
            const double score = (P * R) * (1.0 - fabs(P - R));
            if (in && score > top) {
                top = score;
                top_k = k;
                top_p = P;
                top_r = R;
            }
            const double terms[2] = {t ? P * (R - (double)(ctp - 1) / num_gt) : 0.0, t ? u : 0.0};
            wave_ordered_add<2>(sums, terms);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double o = __shfl_xor(top, m, 64);
            const long long ok = __shfl_xor((long long)top_k, m, 64);
            if (o > top || (o == top && ok < top_k)) {
                top = o;
                top_k = ok;
            }
        }
        const int owner = (int)(top_k & 63);            // n > 0: row top_k was lane top_k & 63's
        const double p = __shfl(top_p, owner, 64), r = __shfl(top_r, owner, 64);
        if (lane == 0) {
            ssd_voc_result out;
            out.ap = n > 0 ? sums[0] : 0.0;
            out.precision = n > 0 ? p : 0.0;
            out.recall = n > 0 ? r : 0.0;
            out.best_threshold = n > 0 ? conf[begin + top_k] : 0.0;
            out.mean_iou = sums[1] / (double)(carry > 1 ? carry : 1);
            out.tp = carry;
            out.best_index = n > 0 ? top_k : 0;
            out.reserved = 0;
            results[l] = out;
        }
    }
}

}  // namespace

extern "C" int ssd_voc_match(const ssd_voc_cell *cells_host, const ssd_voc_cell *cells_dev, int64_t n_cells, const double *det_box_dev,
                             const int32_t *det_pos_dev, int64_t nd, const double *gt_box_dev, int64_t ng, double thr, uint8_t *tp_dev,
                             double *tp_iou_dev, int64_t n_rows, void *stream)
{
    const std::string who = "ssd_voc_match";
    if (n_cells < 0 || n_cells > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": n_cells must be in [0, 2^40]");
    if (nd < 0 || nd > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": nd must be in [0, 2^40]");
    if (ng < 0 || ng > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": ng must be in [0, 2^40]");
    if (n_rows < 0 || n_rows > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": n_rows must be in [0, 2^31 - 1]");
    if (nd > n_rows) return ssd_fail(SSD_ERR_INVALID, who + ": nd must be at most n_rows");
    if (!std::isfinite(thr)) return ssd_fail(SSD_ERR_INVALID, who + ": thr must be finite");
    if (n_cells > 0 && !cells_host) return ssd_fail(SSD_ERR_INVALID, who + ": cells_host is NULL");
    SSDCHK(check_ptrs(who, {{cells_dev, n_cells > 0, 8, "cells_dev"}, {det_box_dev, nd > 0, 8, "det_box_dev"},
                            {det_pos_dev, nd > 0, 4, "det_pos_dev"}, {gt_box_dev, ng > 0, 8, "gt_box_dev"},
                            {tp_dev, nd > 0, 1, "tp_dev"}, {tp_iou_dev, nd > 0, 8, "tp_iou_dev"}}));
    const auto row = [&](int64_t c) { const ssd_voc_cell &x = cells_host[c]; return std::array<int64_t, 4>{x.det_begin, x.D, x.gt_begin, x.G}; };
    int64_t det_end;
    SSDCHK(check_ranges(who, {"cell", "D", "G", -1, SSD_VOC_MAX_GT, true}, n_cells, nd, ng, row, &det_end));
    if (det_end != nd) return ssd_fail(SSD_ERR_INVALID, who + ": the cells' detection ranges end at " + std::to_string(det_end) + ", not at nd");
    if (n_cells == 0) return SSD_OK;
    hipLaunchKernelGGL(voc_match, dim3(wave_grid(n_cells)), dim3(VM_THREADS), 0, (hipStream_t)stream, cells_dev, n_cells, det_box_dev,
                       det_pos_dev, gt_box_dev, thr, tp_dev, tp_iou_dev, n_rows);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

extern "C" int ssd_voc_curve(const ssd_voc_segment *segments_host, const ssd_voc_segment *segments_dev, int32_t n_labels,
                             const uint8_t *tp_dev, const double *tp_iou_dev, const double *conf_dev, int64_t n_rows,
                             ssd_voc_result *results_dev, void *stream)
{
    const std::string who = "ssd_voc_curve";
    if (n_labels < 0 || n_labels > (1 << 24)) return ssd_fail(SSD_ERR_INVALID, who + ": n_labels must be in [0, 2^24]");
    if (n_rows < 0 || n_rows > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": n_rows must be in [0, 2^31 - 1]");
    if (n_labels > 0 && !segments_host) return ssd_fail(SSD_ERR_INVALID, who + ": segments_host is NULL");
    SSDCHK(check_ptrs(who, {{segments_dev, n_labels > 0, 8, "segments_dev"}, {tp_dev, n_rows > 0, 1, "tp_dev"},
                            {tp_iou_dev, n_rows > 0, 8, "tp_iou_dev"}, {conf_dev, n_rows > 0, 8, "conf_dev"},
                            {results_dev, n_labels > 0, 8, "results_dev"}}));
    for (int32_t l = 0; l < n_labels; ++l) {
        const ssd_voc_segment &seg = segments_host[l];
        const auto bad = [&](const char *what) { return ssd_fail(SSD_ERR_INVALID, who + ": segment " + std::to_string(l) + ": " + what); };
        if (seg.count < 0) return bad("count must not be negative");
        if (seg.begin < 0) return bad("begin must not be negative");
        if (seg.begin > n_rows - seg.count) return bad("begin + count runs past n_rows");
        if (seg.num_gt < 1 || seg.num_gt > ((int64_t)1 << 40)) return bad("num_gt must be in [1, 2^40]");
    }
    if (n_labels == 0) return SSD_OK;
    hipLaunchKernelGGL(voc_curve, dim3(wave_grid(n_labels)), dim3(VM_THREADS), 0, (hipStream_t)stream, segments_dev, (int)n_labels, tp_dev,
                       tp_iou_dev, conf_dev, results_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
