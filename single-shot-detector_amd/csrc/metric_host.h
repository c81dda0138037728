// The host side of a wave-per-item launch, which the evaluation entry points share: coco_match.hip, coco_accumulate.hip,
// coco_rows.hip, voc_match.hip and (pointer table and grid cap only) jpeg.hip.  256 lanes per block, one wave per item,
// WAVE_ITEMS items per block, a grid of at most WAVE_GRID_CAP blocks that strides over a table the host has checked.  Here, ONCE:
// the shape's constants, the grid rule, the refusal of a NULL or misaligned device pointer, and the walk over a host table of
// (det_begin, count, gt_begin, count) rows.  Every text is built only for a refusal: a run has tens of thousands of rows.
#pragma once
#include "host.h"

#include <array>
#include <initializer_list>

constexpr int WAVE_ITEMS = 4;                   // waves of a block, one item each
constexpr int WAVE_GRID_CAP = 1024;             // blocks; the rest of the list is grid-strided
// the public header's names for the two, which the Python constants are compared with
static_assert(SSD_COCO_CELLS_PER_BLOCK == WAVE_ITEMS && SSD_VOC_CELLS_PER_BLOCK == WAVE_ITEMS, "one launch shape for the family");
static_assert(SSD_COCO_GRID_CAP == WAVE_GRID_CAP && SSD_VOC_GRID_CAP == WAVE_GRID_CAP, "one launch shape for the family");

static inline unsigned capped_grid(int64_t blocks) { return (unsigned)(blocks < WAVE_GRID_CAP ? blocks : WAVE_GRID_CAP); }
static inline unsigned wave_grid(int64_t items) { return capped_grid((items + WAVE_ITEMS - 1) / WAVE_ITEMS); }

// A device pointer of an entry point: refused when NULL although `need`ed, and when not `align`-byte aligned (a power of two).
struct DevPtr { const void *p; bool need; unsigned align; const char *name; };

// the first pointer of the list that breaks a rule is the one reported, NULL before alignment
static inline int check_ptrs(const std::string &who, std::initializer_list<DevPtr> ptrs)
{
    for (const DevPtr &q : ptrs) {
        if (q.need && !q.p) return ssd_fail(SSD_ERR_INVALID, who + ": " + q.name + " is NULL");
        if ((uintptr_t)q.p & (q.align - 1))
            return ssd_fail(SSD_ERR_INVALID, who + ": " + q.name + " must be " + std::to_string(q.align) + "-byte aligned");
    }
    return SSD_OK;
}

// What a table of ranges calls its rows and their two counts, what the counts may reach (a cap < 0: any count that is not
// negative), and whether the detection ranges must tile [0, nd) from 0 on or only ascend without overlap.
struct RangeTable { const char *row, *det_count, *gt_count; int64_t det_cap, gt_cap; bool det_tile; };

// The walk over the n rows of such a table; read(i) -> {det_begin, detection count, gt_begin, groundtruth count} of row i.
// Per row, in this order: the two counts, the detection range against the row before and against nd, the groundtruth range
// against the row before (ascending, disjoint) and against ng.  -> *det_end: the end of the last detection range (0 for no row).
template <class Read>
int check_ranges(const std::string &who, const RangeTable t, int64_t n, int64_t nd, int64_t ng, Read read, int64_t *det_end)
{
    const int64_t d_max = t.det_cap < 0 ? INT64_MAX : t.det_cap, g_max = t.gt_cap < 0 ? INT64_MAX : t.gt_cap;
    int64_t d_end = 0, g_end = 0;
    for (int64_t i = 0; i < n; ++i) {
        const auto [d0, D, g0, G] = read(i);
        const auto bad = [&, i](const std::string &what) { return ssd_fail(SSD_ERR_INVALID, who + ": " + t.row + " " + std::to_string(i) + ": " + what); };
        const auto count = [&](const std::string &name, int64_t cap) {
            return bad(name + (cap < 0 ? std::string(" must not be negative") : " must be in [0, " + std::to_string(cap) + "]"));
        };
        const auto before = [&](const std::string &does, const char *why) { return bad(does + " the " + t.row + " before (" + why + ")"); };
        if (D < 0 || D > d_max) return count(t.det_count, t.det_cap);
        if (G < 0 || G > g_max) return count(t.gt_count, t.gt_cap);
        if (d0 != d_end && t.det_tile) return before("det_begin must be the end of", "the detection ranges tile [0, nd)");
        if (d0 < d_end) return before("det_begin overlaps", "ranges ascend and are disjoint");
        if (d0 > nd - D) return bad(std::string("det_begin + ") + t.det_count + " runs past nd");
        if (g0 < g_end) return before("gt_begin overlaps", "ranges ascend and are disjoint");
        if (g0 > ng - G) return bad(std::string("gt_begin + ") + t.gt_count + " runs past ng");
        d_end = d0 + D, g_end = g0 + G;
    }
    *det_end = d_end;
    return SSD_OK;
}
