// The COCO box matching: CocoBoxEval.evaluate() (coco_metric.py) for every cell of a run in one launch.  Semantics, the packed
// layout and every refusal: include/ssd_hip.h, block "the COCO box matching".
//
//   coco_match   256 lanes per block, one wave per cell, SSD_COCO_CELLS_PER_BLOCK (4) cells per block; a grid of at most
//                SSD_COCO_GRID_CAP blocks strides over the cell list.  Every wave of a block makes the same number of passes (a wave
//                behind the list's end only meets the barriers), so the two __syncthreads of a pass are block-uniform.
//                The 64 lanes stage the cell's detection boxes and its groundtruth boxes, areas and crowd bytes in LDS as they
//                are (float64).  Lane a * T + t then runs the scan of area range a at threshold t alone; lanes from T * A on only help
//                with staging and stores.  The loops over d and g are wave-uniform: every lane forms IoU(d, g) from the same LDS
//                words with the same operations, so all lanes compare the same float64 bits, and what differs between lanes (the
//                ignore flag, taken, best, m) is predicated.  The scan order is two passes over g in annotation order -- the boxes that
//                are not ignored, then the ignored ones -- which is the stable sort by the flag without storing a permutation.  `taken` is
//                a bit mask per lane in LDS, word-major ([g / 32][lane]: a lane touches its own column only, no bank conflict).
//                Per detection one ballot each collects `matched` and `ignored` of the 64 lanes; lane a < A shifts out the T bits
//                of its area range and stores one uint16.  gt_ignore in scan order is `j >= number of boxes not ignored`, written by
//                the whole wave; so is the optional IoU dump, whose offset (the sum of D * G over the cells before) every wave
//                carries forward from its previous cell.  No atomics; 62 976 bytes of LDS per block.
#include "metric_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_WAVES = SSD_COCO_CELLS_PER_BLOCK;
constexpr int CM_TAKEN_WORDS = SSD_COCO_MAX_GT / 32;
static_assert(CM_THREADS == 64 * CM_WAVES, "one wave per cell");
static_assert(SSD_COCO_MAX_GT % 32 == 0, "taken is whole 32-bit words");
static_assert(sizeof(ssd_coco_cell) == 24 && offsetof(ssd_coco_cell, gt_begin) == 8 && offsetof(ssd_coco_cell, D) == 16 &&
              offsetof(ssd_coco_cell, G) == 20, "ssd_coco_cell is the 24-byte row of include/ssd_hip.h");

struct CocoParams {
    double thr[SSD_COCO_MAX_THR];
    double rng[SSD_COCO_MAX_AREA][2];
};

// bbox_iou of coco_metric.py on one pair: every operation rounded once, the division correctly rounded
__device__ __forceinline__ double iou_xywh(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh, bool crowd)
{
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    if (!(w > 0.0 && h > 0.0)) return 0.0;
    const double inter = w * h;
    const double da = dw * dh;
    const double ga = gw * gh;
    const double uni = crowd ? da : (da + ga) - inter;
    return inter / uni;
}

__global__ __launch_bounds__(CM_THREADS) void coco_match(const ssd_coco_cell *__restrict__ cells, int64_t n_cells,
                                                         const double *__restrict__ det_box, const double *__restrict__ det_area, int64_t nd,
                                                         const double *__restrict__ gt_box, const double *__restrict__ gt_area,
                                                         const uint8_t *__restrict__ gt_crowd, int64_t ng, CocoParams p, int T, int A,
                                                         uint16_t *__restrict__ matched, uint16_t *__restrict__ ignored,
                                                         uint8_t *__restrict__ gt_ignore, double *__restrict__ iou_out)
{
    __shared__ double s_dbox[CM_WAVES][SSD_COCO_MAX_DET * 4];
    __shared__ double s_gbox[CM_WAVES][SSD_COCO_MAX_GT * 4];
    __shared__ double s_garea[CM_WAVES][SSD_COCO_MAX_GT];
    __shared__ unsigned s_taken[CM_WAVES][CM_TAKEN_WORDS][64];
    __shared__ uint8_t s_crowd[CM_WAVES][SSD_COCO_MAX_GT];

    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const bool scans = lane < T * A;
    const int a = scans ? lane / T : 0, t = scans ? lane - a * T : 0;
    // this lane's threshold and bounds, picked by compares: no lane-indexed read of the argument block
    double thr = p.thr[0], lo = p.rng[0][0], hi = p.rng[0][1];
#pragma unroll
    for (int k = 1; k < SSD_COCO_MAX_THR; ++k) thr = t == k ? p.thr[k] : thr;
#pragma unroll
    for (int k = 1; k < SSD_COCO_MAX_AREA; ++k) {
        lo = a == k ? p.rng[k][0] : lo;
        hi = a == k ? p.rng[k][1] : hi;
    }
    const unsigned long long tmask = (1ull << T) - 1ull;

    double *dbox = s_dbox[wave], *gbox = s_gbox[wave], *garea = s_garea[wave];
    uint8_t *crowd = s_crowd[wave];

    const int64_t stride = (int64_t)gridDim.x * CM_WAVES;
    int64_t iou_off = 0, prev = 0;                      // the dump's offset of cell `prev`
    for (int64_t base = (int64_t)blockIdx.x * CM_WAVES; base < n_cells; base += stride) {
        const int64_t c = base + wave;
        const bool live = c < n_cells;                  // wave-uniform
        int D = 0, G = 0;
        int64_t d0 = 0, g0 = 0;
        if (live) {
            const ssd_coco_cell cell = cells[c];
            D = cell.D; G = cell.G; d0 = cell.det_begin; g0 = cell.gt_begin;
            for (int i = lane; i < D * 4; i += 64) dbox[i] = det_box[d0 * 4 + i];
            for (int i = lane; i < G * 4; i += 64) gbox[i] = gt_box[g0 * 4 + i];
            for (int i = lane; i < G; i += 64) {
                garea[i] = gt_area[g0 + i];
                crowd[i] = gt_crowd[g0 + i];
            }
#pragma unroll
            for (int w = 0; w < CM_TAKEN_WORDS; ++w) s_taken[wave][w][lane] = 0u;
        }
        __syncthreads();
        if (live) {
            // ---- gt_ignore in scan order: the boxes that are not ignored come first
            for (int k = 0; k < A; ++k) {
                double klo = p.rng[0][0], khi = p.rng[0][1];
#pragma unroll
                for (int q = 1; q < SSD_COCO_MAX_AREA; ++q) {
                    klo = k == q ? p.rng[q][0] : klo;
                    khi = k == q ? p.rng[q][1] : khi;
                }
                int regular = 0;
                for (int gb = 0; gb < G; gb += 64) {
                    const int g = gb + lane;
                    const bool reg = g < G && !(crowd[g] != 0 || garea[g] < klo || garea[g] > khi);
                    regular += __popcll(__ballot(reg));
                }
                for (int j = lane; j < G; j += 64) gt_ignore[(int64_t)k * ng + g0 + j] = j >= regular ? 1 : 0;
            }
            // ---- the optional IoU dump, [D, G] in annotation order behind the blocks of the cells before
            if (iou_out) {
                int64_t part = 0;
                for (int64_t k = prev + lane; k < c; k += 64) part += (int64_t)cells[k].D * (int64_t)cells[k].G;
                for (int m = 1; m < 64; m <<= 1) part += __shfl_xor(part, m, 64);
                iou_off += part;
                prev = c;
                for (int i = lane; i < D * G; i += 64) {
                    const int d = i / G, g = i - d * G;
                    iou_out[iou_off + i] = iou_xywh(dbox[d * 4], dbox[d * 4 + 1], dbox[d * 4 + 2], dbox[d * 4 + 3], gbox[g * 4],
                                                    gbox[g * 4 + 1], gbox[g * 4 + 2], gbox[g * 4 + 3], crowd[g] != 0);
                }
            }
            // ---- the scans: lane a * T + t alone, d and g wave-uniform
            for (int d = 0; d < D; ++d) {
                const double dx = dbox[d * 4], dy = dbox[d * 4 + 1], dw = dbox[d * 4 + 2], dh = dbox[d * 4 + 3];
                double best = thr;
                int m = -1;
                bool m_ig = false, stop = false;
                for (int pass = 0; pass < 2; ++pass) {
                    for (int g = 0; g < G; ++g) {
                        const bool cr = crowd[g] != 0;
                        const double ga = garea[g];
                        const double iou = iou_xywh(dx, dy, dw, dh, gbox[g * 4], gbox[g * 4 + 1], gbox[g * 4 + 2], gbox[g * 4 + 3], cr);
                        const bool ig = cr || ga < lo || ga > hi;
                        const bool tk = (s_taken[wave][g >> 5][lane] >> (g & 31)) & 1u;
                        bool visit = scans && !stop && ig == (pass == 1) && !(tk && !cr);
                        if (visit && m >= 0 && !m_ig && ig) {       // a regular match is held: the scan ends
                            stop = true;
                            visit = false;
                        }
                        if (visit && !(iou < best)) {
                            best = iou;
                            m = g;
                            m_ig = ig;
                        }
                    }
                }
                const bool hit = scans && m >= 0;
                if (hit) s_taken[wave][m >> 5][lane] |= 1u << (m & 31);
                const double da = det_area[d0 + d];
                const bool ign = scans && (hit ? m_ig : (da < lo || da > hi));
                const unsigned long long mb = __ballot(hit), ib = __ballot(ign);
                if (lane < A) {
                    matched[(int64_t)lane * nd + d0 + d] = (uint16_t)((mb >> (lane * T)) & tmask);
                    ignored[(int64_t)lane * nd + d0 + d] = (uint16_t)((ib >> (lane * T)) & tmask);
                }
            }
        }
        __syncthreads();                                // the next pass's staging overwrites what this pass read
    }
}

}  // namespace

extern "C" int ssd_coco_match(const ssd_coco_cell *cells_host, const ssd_coco_cell *cells_dev, int64_t n_cells,
                              const double *det_box_dev, const double *det_area_dev, int64_t nd,
                              const double *gt_box_dev, const double *gt_area_dev, const uint8_t *gt_crowd_dev, int64_t ng,
                              const double *thr_host, int32_t T, const double *area_rng_host, int32_t A,
                              uint16_t *matched_dev, uint16_t *ignored_dev, uint8_t *gt_ignore_dev, double *iou_dev, void *stream)
{
    const std::string who = "ssd_coco_match";
    if (n_cells < 0 || n_cells > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": n_cells must be in [0, 2^40]");
    if (nd < 0 || nd > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": nd must be in [0, 2^40]");
    if (ng < 0 || ng > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, who + ": ng must be in [0, 2^40]");
    if (!thr_host) return ssd_fail(SSD_ERR_INVALID, who + ": thr_host is NULL");
    if (!area_rng_host) return ssd_fail(SSD_ERR_INVALID, who + ": area_rng_host is NULL");
    const std::string t_range = who + ": T must be in [1, " + std::to_string(SSD_COCO_MAX_THR) + "]";
    const std::string a_range = who + ": A must be in [1, " + std::to_string(SSD_COCO_MAX_AREA) + "]";
    if (T < 1) return ssd_fail(SSD_ERR_INVALID, t_range);
    if (A < 1) return ssd_fail(SSD_ERR_INVALID, a_range);
    if ((int64_t)T * A > 64) return ssd_fail(SSD_ERR_INVALID, who + ": T * A must be at most 64, one lane per scan");
    if (T > SSD_COCO_MAX_THR) return ssd_fail(SSD_ERR_INVALID, t_range);
    if (A > SSD_COCO_MAX_AREA) return ssd_fail(SSD_ERR_INVALID, a_range);
    if (n_cells > 0 && !cells_host) return ssd_fail(SSD_ERR_INVALID, who + ": cells_host is NULL");
    SSDCHK(check_ptrs(who, {{cells_dev, n_cells > 0, 8, "cells_dev"}, {det_box_dev, nd > 0, 8, "det_box_dev"},
                            {det_area_dev, nd > 0, 8, "det_area_dev"}, {gt_box_dev, ng > 0, 8, "gt_box_dev"},
                            {gt_area_dev, ng > 0, 8, "gt_area_dev"}, {gt_crowd_dev, ng > 0, 1, "gt_crowd_dev"},
                            {matched_dev, nd > 0, 2, "matched_dev"}, {ignored_dev, nd > 0, 2, "ignored_dev"},
                            {gt_ignore_dev, ng > 0, 1, "gt_ignore_dev"}, {iou_dev, false, 8, "iou_dev"}}));
    const auto row = [&](int64_t c) { const ssd_coco_cell &x = cells_host[c]; return std::array<int64_t, 4>{x.det_begin, x.D, x.gt_begin, x.G}; };
    int64_t det_end;
    SSDCHK(check_ranges(who, {"cell", "D", "G", SSD_COCO_MAX_DET, SSD_COCO_MAX_GT, false}, n_cells, nd, ng, row, &det_end));
    if (n_cells == 0) return SSD_OK;
    CocoParams p;
    for (int k = 0; k < SSD_COCO_MAX_THR; ++k) p.thr[k] = thr_host[k < T ? k : 0];
    for (int k = 0; k < SSD_COCO_MAX_AREA; ++k) {
        p.rng[k][0] = area_rng_host[2 * (k < A ? k : 0)];
        p.rng[k][1] = area_rng_host[2 * (k < A ? k : 0) + 1];
    }
    hipLaunchKernelGGL(coco_match, dim3(wave_grid(n_cells)), dim3(CM_THREADS), 0, (hipStream_t)stream, cells_dev, n_cells, det_box_dev, det_area_dev, nd,
                       gt_box_dev, gt_area_dev, gt_crowd_dev, ng, p, (int)T, (int)A, matched_dev, ignored_dev, gt_ignore_dev, iou_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
