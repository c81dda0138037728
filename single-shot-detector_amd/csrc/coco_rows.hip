// The COCO rows: the inputs of ssd_coco_match built from the engine's record blocks, for every image of a run in two launches.
// Semantics, the layout and every refusal: include/ssd_hip.h, block "the COCO rows".
//
//   coco_rows<FILL>   256 lanes per block, one wave per image, SSD_COCO_CELLS_PER_BLOCK (4) of them per block; a grid of at most
//                     SSD_COCO_GRID_CAP blocks strides over the images.  The waves of a block share nothing but the block's LDS, each its
//                     own 2 * T words: no __syncthreads, every wave makes its own number of passes.
//                     A wave walks its image's live rows (j < num_boxes) 64 at a time.  A lane forms its row's verdict -- kept, its
//                     category index, bad -- and the kept rows go to the wave's LDS compacted in row order (one ballot per chunk):
//                     score [n_kept] | category [n_kept].  Everything later reads that list with wave-uniform addresses (broadcasts).
//                       count   lane k counts the list's entries of category k (k = lane, lane + 64, ..) and stores min(count, 100):
//                               every counts[k, i] is written once, zeros included; the lowest bad row by a minimum over the lanes.
//                       fill    the walk again (the verdicts recomputed from the same words): a kept row's rank is the number of
//                               list entries of its category that come before it -- a larger score, or an equal one at a smaller list
//                               position, which is a smaller record row --, and a rank below 100 stores the row at det_begin[k, i] +
//                               rank if that lies in [0, nd).  No sort, no atomics.
//                     The four products and the two differences of a box are single float32 operations (__fmul_rn / __fsub_rn, and
//                     contraction is off for the file): fusing a product into the subtraction changes w or h of a few boxes per million.
#include "metric_host.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = SSD_COCO_CELLS_PER_BLOCK;
static_assert(CR_THREADS == 64 * CR_WAVES, "one wave per image");
static_assert((size_t)CR_WAVES * 2 * SSD_COCO_ROWS_MAX_T * 4 <= 65536, "the waves' lists fit the LDS a launch gets without asking");

struct RowArgs {
    const int32_t *records;
    int64_t n_images;
    int T;
    const int32_t *image_hw, *label_to_cat;
    int num_labels, K;
    float thr;
};

struct Row {
    float score, x, y, w, h;        // x .. h: already truncated toward zero
    int cat;                        // the category index of a kept row, -1 for every other row
    bool bad;
};

// row j of the record at `rec` (include/ssd_hip.h: "Row semantics"); j >= num is no row at all
__device__ __forceinline__ Row load_row(const RowArgs &a, const int32_t *__restrict__ rec, int j, int num, float H, float W)
{
    Row r;
    r.score = r.x = r.y = r.w = r.h = 0.0f;
    r.cat = -1;
    r.bad = false;
    if (j >= num) return r;
    const float s = __int_as_float(rec[4 * a.T + j]);
    r.score = s;
    if (!__builtin_isfinite(s)) {
        r.bad = true;
        return r;
    }
    if (!(s > a.thr)) return r;
    const int label = rec[5 * a.T + j];
    const float py0 = __fmul_rn(__int_as_float(rec[4 * j + 0]), H), px0 = __fmul_rn(__int_as_float(rec[4 * j + 1]), W);
    const float py1 = __fmul_rn(__int_as_float(rec[4 * j + 2]), H), px1 = __fmul_rn(__int_as_float(rec[4 * j + 3]), W);
    const float lim = 0x1p30f;      // (a NaN or an infinity fails every comparison)
    const bool box_ok = fabsf(py0) < lim && fabsf(px0) < lim && fabsf(py1) < lim && fabsf(px1) < lim;
    if (!box_ok || (unsigned)label >= (unsigned)a.num_labels) {
        r.bad = true;
        return r;
    }
    const int cat = a.label_to_cat[label];
    r.cat = (unsigned)cat < (unsigned)a.K ? cat : -1;
    r.x = truncf(px0);
    r.y = truncf(py0);
    r.w = truncf(__fsub_rn(px1, px0));
    r.h = truncf(__fsub_rn(py1, py0));
    return r;
}

typedef double double2_t __attribute__((ext_vector_type(2)));

template <bool FILL>
__global__ __launch_bounds__(CR_THREADS) void coco_rows(RowArgs a, int32_t *__restrict__ counts, int32_t *__restrict__ bad,
                                                        const int64_t *__restrict__ det_begin, int64_t nd, double *__restrict__ det_box,
                                                        double *__restrict__ det_area, double *__restrict__ det_score, int box16)
{
    extern __shared__ uint32_t s_lists[];

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    float *s_score = reinterpret_cast<float *>(s_lists + (size_t)wave * 2 * a.T);
    int *s_cat = reinterpret_cast<int *>(s_lists + (size_t)wave * 2 * a.T + a.T);
    const unsigned long long below = (1ull << lane) - 1ull;        // the lanes in front of this one
    const int64_t words = 6 * (int64_t)a.T + 1, stride = (int64_t)gridDim.x * CR_WAVES;
    for (int64_t img = (int64_t)blockIdx.x * CR_WAVES + wave; img < a.n_images; img += stride) {
        const int32_t *__restrict__ rec = a.records + img * words;
        const int num_raw = rec[6 * a.T];
        const bool num_ok = num_raw >= 0 && num_raw <= a.T;
        const int num = num_ok ? num_raw : 0;
        const float H = (float)a.image_hw[2 * img], W = (float)a.image_hw[2 * img + 1];

        // ---- the kept rows, compacted in row order
        int first_bad = num_ok ? INT_MAX : a.T, n_kept = 0;
        wave_lds_sync();                                    // the reads of the image before are done
        for (int j0 = 0; j0 < num; j0 += 64) {
            const int j = j0 + lane;
            const Row r = load_row(a, rec, j, num, H, W);
            if (r.bad) first_bad = min(first_bad, j);
            const unsigned long long m = __ballot(r.cat >= 0);
            if (r.cat >= 0) {
                const int p = n_kept + __popcll(m & below);      // p <= j < T
                s_score[p] = r.score;
                s_cat[p] = r.cat;
            }
            n_kept += __popcll(m);
        }
        wave_lds_sync();

        if (!FILL) {
            for (int k0 = 0; k0 < a.K; k0 += 64) {
                const int k = k0 + lane;
                int c = 0;
                for (int p = 0; p < n_kept; ++p) c += s_cat[p] == k ? 1 : 0;
                if (k < a.K) counts[(int64_t)k * a.n_images + img] = min(c, SSD_COCO_MAX_DET);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) first_bad = min(first_bad, __shfl_xor(first_bad, d, 64));
            if (lane == 0) bad[img] = first_bad == INT_MAX ? -1 : first_bad;
            continue;
        }

        // ---- fill: the walk again, every kept row to its rank
        int front = 0;                                      // list entries of the chunks before
        for (int j0 = 0; j0 < num; j0 += 64) {
            const Row r = load_row(a, rec, j0 + lane, num, H, W);
            const unsigned long long m = __ballot(r.cat >= 0);
            if (m == 0) continue;
            const int p = front + __popcll(m & below);
            front += __popcll(m);
            int rank = 0;
            for (int q = 0; q < n_kept; ++q) {
                const float sq = s_score[q];
                rank += s_cat[q] == r.cat && (sq > r.score || (sq == r.score && q < p)) ? 1 : 0;
            }
            if (r.cat >= 0 && rank < SSD_COCO_MAX_DET) {
                const int64_t at = det_begin[(int64_t)r.cat * a.n_images + img] + rank;
                if (at >= 0 && at < nd) {                   // (a table that is not the counts' scan: no store outside the arrays)
                    const double x = (double)r.x, y = (double)r.y, w = (double)r.w, h = (double)r.h;
                    double *row = det_box + 4 * at;
                    if (box16) {
                        double2_t lo, hi;
                        lo.x = x, lo.y = y, hi.x = w, hi.y = h;
                        *reinterpret_cast<double2_t *>(row) = lo;
                        *reinterpret_cast<double2_t *>(row + 2) = hi;
                    } else {
                        row[0] = x, row[1] = y, row[2] = w, row[3] = h;
                    }
                    det_area[at] = (double)((long long)r.w * (long long)r.h);
                    det_score[at] = (double)r.score;
                }
            }
        }
    }
}

// what both entry points refuse: SSD_OK, or the recorded failure
int check_rows(const std::string &who, const int32_t *records_dev, int64_t n_images, int32_t T, const int32_t *image_hw_dev,
               const int32_t *label_to_cat_dev, int32_t num_labels, int32_t K, float score_threshold)
{
    if (n_images < 0 || n_images > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": n_images must be in [0, 2^31 - 1]");
    if (T < 1 || T > SSD_COCO_ROWS_MAX_T)
        return ssd_fail(SSD_ERR_INVALID, who + ": T must be in [1, " + std::to_string(SSD_COCO_ROWS_MAX_T) + "]");
    if (K < 1 || K > (1 << 20)) return ssd_fail(SSD_ERR_INVALID, who + ": K must be in [1, 2^20]");
    if ((int64_t)K * n_images > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": K * n_images must not pass 2^31 - 1");
    if (num_labels < 1 || num_labels > (1 << 20)) return ssd_fail(SSD_ERR_INVALID, who + ": num_labels must be in [1, 2^20]");
    if (!std::isfinite(score_threshold)) return ssd_fail(SSD_ERR_INVALID, who + ": score_threshold must be finite");
    return check_ptrs(who, {{records_dev, n_images > 0, 4, "records_dev"}, {image_hw_dev, n_images > 0, 4, "image_hw_dev"},
                            {label_to_cat_dev, n_images > 0, 4, "label_to_cat_dev"}});
}

}  // namespace

extern "C" int ssd_coco_rows_count(const int32_t *records_dev, int64_t n_images, int32_t T, const int32_t *image_hw_dev,
                                   const int32_t *label_to_cat_dev, int32_t num_labels, int32_t K, float score_threshold,
                                   int32_t *counts_dev, int32_t *bad_dev, void *stream)
{
    const std::string who = "ssd_coco_rows_count";
    SSDCHK(check_rows(who, records_dev, n_images, T, image_hw_dev, label_to_cat_dev, num_labels, K, score_threshold));
    SSDCHK(check_ptrs(who, {{counts_dev, n_images > 0, 4, "counts_dev"}, {bad_dev, n_images > 0, 4, "bad_dev"}}));
    if (n_images == 0) return SSD_OK;
    const RowArgs a = {records_dev, n_images, (int)T, image_hw_dev, label_to_cat_dev, (int)num_labels, (int)K, score_threshold};
    hipLaunchKernelGGL(coco_rows<false>, dim3(wave_grid(n_images)), dim3(CR_THREADS), (size_t)CR_WAVES * 2 * T * 4, (hipStream_t)stream, a,
                       counts_dev, bad_dev, (const int64_t *)nullptr, (int64_t)0, (double *)nullptr, (double *)nullptr, (double *)nullptr, 0);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

extern "C" int ssd_coco_rows_fill(const int32_t *records_dev, int64_t n_images, int32_t T, const int32_t *image_hw_dev,
                                  const int32_t *label_to_cat_dev, int32_t num_labels, int32_t K, float score_threshold,
                                  const int64_t *det_begin_dev, int64_t nd, double *det_box_dev, double *det_area_dev,
                                  double *det_score_dev, void *stream)
{
    const std::string who = "ssd_coco_rows_fill";
    SSDCHK(check_rows(who, records_dev, n_images, T, image_hw_dev, label_to_cat_dev, num_labels, K, score_threshold));
    if (nd < 0 || nd > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": nd must be in [0, 2^31 - 1]");
    const bool rows = n_images > 0 && nd > 0;
    SSDCHK(check_ptrs(who, {{det_begin_dev, n_images > 0, 8, "det_begin_dev"}, {det_box_dev, rows, 8, "det_box_dev"},
                            {det_area_dev, rows, 8, "det_area_dev"}, {det_score_dev, rows, 8, "det_score_dev"}}));
    if (n_images == 0 || nd == 0) return SSD_OK;            // no row of any image has a place
    const RowArgs a = {records_dev, n_images, (int)T, image_hw_dev, label_to_cat_dev, (int)num_labels, (int)K, score_threshold};
    hipLaunchKernelGGL(coco_rows<true>, dim3(wave_grid(n_images)), dim3(CR_THREADS), (size_t)CR_WAVES * 2 * T * 4, (hipStream_t)stream, a,
                       (int32_t *)nullptr, (int32_t *)nullptr, det_begin_dev, nd, det_box_dev, det_area_dev, det_score_dev,
                       ((uintptr_t)det_box_dev & 15) == 0 ? 1 : 0);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
