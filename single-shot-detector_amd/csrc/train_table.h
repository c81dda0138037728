// What the four table kernels at the end of the TRAIN step share: update.hip (Adam + EMA), train_norms.hip, train_hist.hip and
// train_reduce.hip (the gradient exchange).  All four cut their table into blocks of SSD_UPDATE_BLOCK_ELEMS elements, 256 lanes per
// block, lane t on the quads (k * 256 + t) * 4, k = 0..3, under a grid of at most TBL_MAX_GRID blocks that strides over the work
// list.  Here, ONCE: the shape's constants, the host checks of an ssd_update_tensor table and of a workspace, the block-uniform row
// search, the read-side walk of one block, and the two pieces that carry the ORDER of the double additions (include/ssd_hip.h,
// blocks "the TRAIN step's norms" and "the TRAIN step's histograms"): the 256-lane tree and stage 2's ascending chain.
#pragma once
#include "host.h"

typedef float v4f __attribute__((ext_vector_type(4)));
// the rows hold plain pointers, whose address space the compiler cannot know: said to be global memory, the kernels' loads and
// stores are global_load / global_store instead of flat ones
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) v4f gv4f;

constexpr int TBL_THREADS = 256;
constexpr int TBL_QUADS = 4;                                        // 16-byte groups per lane and block
constexpr int TBL_STEP = TBL_THREADS * 4;                           // elements one pass of the 256 lanes covers
constexpr int TBL_MAX_GRID = 2048;                                  // 256 CUs x 8 blocks: the rest is grid-strided
constexpr int TBL_WAVE = 64;                                        // stage 2: one wave per tensor
static_assert(TBL_QUADS * TBL_STEP == SSD_UPDATE_BLOCK_ELEMS, "a block is 256 lanes x 4 quads x 4 elements");
static_assert(sizeof(ssd_update_tensor) == 56, "ssd_update_tensor is the 56-byte row of include/ssd_hip.h");

static inline unsigned grid_for(int64_t blocks) { return (unsigned)(blocks < TBL_MAX_GRID ? blocks : TBL_MAX_GRID); }

// ----------------------------------------------------------------------------- host checks (defined in update.hip)
// The refusals of an ssd_update_tensor table, every text behind "<fn>: ".  check_update_args: the tables themselves (`others`: the
// caller's further pointers that are refused together with them), T, tensors_dev's alignment; check_update_rows: every row, in order
// -> the table's blocks; check_update_table: the one, then the other.
int check_update_args(const char *fn, const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, bool others = true);
int check_update_rows(const char *fn, const ssd_update_tensor *tensors_host, int32_t T, int64_t *blocks_out);
int check_update_table(const char *fn, const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, int64_t *blocks_out);
// a planner: block_bytes per block of the table, 0 for a table that is refused (the planner sees no device table)
size_t update_table_bytes(const char *fn, const ssd_update_tensor *tensors_host, int32_t T, size_t block_bytes);
// the workspace of such a plan: NULL, not 16-byte aligned, smaller than `needs`
int check_workspace(const char *fn, const void *workspace, size_t workspace_bytes, size_t needs);

// ----------------------------------------------------------------------------- the row of a block
// The last row whose key <= c (key_0 == 0 <= c).  Of rows that share a key -- a row of no blocks and its successor -- that is the
// last, so an empty row in front of one with blocks is never found.  c is block-uniform: the search and the row are scalar loads.
template <class Row, class Key>
__device__ __forceinline__ int row_of_block(const Row *__restrict__ rows, int T, Key Row::*key, Key c)
{
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].*key <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// ----------------------------------------------------------------------------- the read-side walk of one block
// Virtual elements [j0, j0 + 4096) of a tensor, counted from the 16-byte boundary at or below w (the first `pad` lie before the
// tensor, [pad, pad + count) are the tensor): f(x, g, in) for this lane's 16 elements, quad k = 0..3, element e = 0..3, in that
// order; x of w, g of grad (+0.0f without GRAD).  w's quads are always 16-byte aligned, grad's where grad is congruent to w modulo
// 16 (gvec).  A block wholly inside the tensor (with GRAD: and gvec) issues its 4 (8) 16-byte loads before the first f.  Any other
// block -- the tensor's head or tail, a gradient of another alignment class -- takes whole quads where they fit and are aligned and
// single elements otherwise, always INTO the quad's own lane, so nothing a caller sums depends on the load width; there every lane
// visits all 16 positions and an element outside the tensor arrives as +0.0f with in == false (a caller's ballots see the whole
// wave).  No address outside [w, w + count) or [grad, grad + count) is read.
template <bool GRAD, class F>
__device__ __forceinline__ void walk_block(const gfloat *w, const gfloat *grad, int64_t count, int64_t j0, int pad, bool gvec, F f)
{
    const int tid = (int)threadIdx.x;
    const int64_t end = pad + count;
    if (j0 >= pad && j0 + SSD_UPDATE_BLOCK_ELEMS <= end && (!GRAD || gvec)) {
        const int64_t i0 = j0 - pad + tid * 4;
        v4f x[TBL_QUADS], g[TBL_QUADS];
#pragma unroll
        for (int k = 0; k < TBL_QUADS; ++k) {
            const int64_t i = i0 + k * TBL_STEP;
            x[k] = *(const gv4f *)(w + i);
            if (GRAD) g[k] = *(const gv4f *)(grad + i);
            else g[k] = (v4f){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < TBL_QUADS; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) f(x[k][e], g[k][e], true);
    } else {
#pragma unroll 1
        for (int k = 0; k < TBL_QUADS; ++k) {
            const int64_t j = j0 + (int64_t)(k * TBL_THREADS + tid) * 4;
            const bool whole = j >= pad && j + 4 <= end;
            v4f x = (v4f){0.f, 0.f, 0.f, 0.f}, g = (v4f){0.f, 0.f, 0.f, 0.f};
            if (whole) {
                x = *(const gv4f *)(w + (j - pad));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e >= pad && j + e < end) x[e] = w[j + e - pad];
            }
            if (GRAD) {
                if (whole && gvec) {
                    g = *(const gv4f *)(grad + (j - pad));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e >= pad && j + e < end) g[e] = grad[j + e - pad];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) f(x[e], g[e], j + e >= pad && j + e < end);
        }
    }
}

// ----------------------------------------------------------------------------- the order of the double additions
// The 256-lane tree a[t] += a[t + s] on N doubles per lane: s = 128 and 64 across the four waves through LDS (wave 0 reads four
// values and adds them as (a[t] + a[t+128]) + (a[t+64] + a[t+192])), s = 32 .. 1 inside wave 0 with cross-lane moves.  On return
// lane 0 holds the block's sums.  The barrier between the two halves is the block's: what the caller stored to LDS before the call
// (its integer companions) can be read behind it; the caller places the barrier that lets `lds` be written again.
template <int N>
__device__ __forceinline__ void tree256(double (&v)[N], double (&lds)[N][TBL_THREADS])
{
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < N; ++q) lds[q][tid] = v[q];
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = (lds[q][tid] + lds[q][tid + 128]) + (lds[q][tid + 64] + lds[q][tid + 192]);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int q = 0; q < N; ++q) v[q] = v[q] + __shfl_down(v[q], s, 64);
    }
}

// Stage 2, one wave per tensor: the lanes hold 64 consecutive blocks' partials v (fetched at once, all in flight together); every
// lane adds the 64 to s in ascending lane order, reading lane i's value with v_readlane (a constant lane: the loop is unrolled), so
// that the chain of dependent double additions is all that is serial.  A lane past the tensor's last block holds +0.0, which leaves
// a sum that started at +0.0 as it is (a sum of these calls is never -0.0: +0.0 + -0.0 = +0.0).  (One lane per tensor walking its
// blocks alone waits out a memory latency every few partials, and cross-lane reads through the LDS crossbar a round trip per
// partial: the largest tensors have 256 blocks.)
template <int N>
__device__ __forceinline__ void wave_ordered_add(double (&s)[N], const double (&v)[N])
{
    int lo[N], hi[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        lo[q] = __double2loint(v[q]);
        hi[q] = __double2hiint(v[q]);
    }
#pragma unroll
    for (int i = 0; i < TBL_WAVE; ++i)
#pragma unroll
        for (int q = 0; q < N; ++q)
            s[q] = s[q] + __hiloint2double(__builtin_amdgcn_readlane(hi[q], i), __builtin_amdgcn_readlane(lo[q], i));
}
