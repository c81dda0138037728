// The TRAIN step's norms: sum w^2, sum g^2 and the non-finite counts of every tensor of the update's table, before the update
// consumes the gradients.  Semantics and the ORDER of the double additions: include/ssd_hip.h, block "the TRAIN step's norms".
//
//   train_norms_blocks   stage 1, update.hip's shape: 256 lanes per block, the work list is the model cut into blocks of
//                        SSD_UPDATE_BLOCK_ELEMS virtual elements counted from the 16-byte boundary at or below w, a grid of at most
//                        NRM_MAX_GRID blocks strides over it; the row is found by the same block-uniform binary search over
//                        first_block, so the search and the row are scalar loads and every branch on the row (gradient present,
//                        its alignment class, whole block inside the tensor) is taken by all lanes alike.  Lane t owns the quads
//                        j0 + (k * 256 + t) * 4, k = 0..3: w's quads are always 16-byte aligned (pad is w's offset in its group),
//                        grad's where grad is congruent to w modulo 16.  A block wholly inside the tensor issues its 4 (8 with such
//                        a gradient) 16-byte loads before the arithmetic; the blocks with the tensor's head or tail check each quad
//                        and take single elements where a quad crosses an end; a gradient of another alignment class is read
//                        element by element INTO the same lane's quad, so the sums do not depend on the load width.  The 256 lane
//                        values go through the header's tree: s = 128, 64 across the four waves through LDS (wave 0 reads four
//                        values and adds them as (a[t] + a[t+128]) + (a[t+64] + a[t+192])), s = 32 .. 1 inside wave 0 with
//                        cross-lane moves.  Lane 0 writes the block's 32-byte partial with two 16-byte vector stores.
//   train_norms_rows     stage 2: one wave per tensor loads 64 of its blocks' partials at a time and adds them in ascending block
//                        order.
// No atomics; reads w and grad, writes the workspace and the outputs only.
#include "host.h"

#include <cmath>

#pragma clang fp contract(off)

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) const v4f gcv4f;

namespace {

constexpr int NRM_THREADS = 256;
constexpr int NRM_QUADS = 4;                                        // 16-byte groups per lane and block
constexpr int NRM_MAX_GRID = 2048;                                  // 256 CUs x 8 blocks: the rest is grid-strided
constexpr int NRM_ROW_THREADS = 64;
static_assert(NRM_THREADS * NRM_QUADS * 4 == SSD_UPDATE_BLOCK_ELEMS, "a block is 256 lanes x 4 quads x 4 elements");
static_assert(sizeof(ssd_update_tensor) == 56, "ssd_update_tensor is the 56-byte row of include/ssd_hip.h");

struct Partial {                                                    // SSD_NORMS_BLOCK_BYTES: one block's, and one row's, result
    double sw, sg;
    long long bw, bg;
};
static_assert(sizeof(Partial) == SSD_NORMS_BLOCK_BYTES, "a partial is two doubles and two int64");

// the header's arithmetic on one element: the exact square in double, or +0.0 and a count for NaN / +-inf
__device__ __forceinline__ void norm_one(float x, double &sum, int &bad)
{
    const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    const double d = (double)x;
    sum = sum + (finite ? d * d : 0.0);
    bad += finite ? 0 : 1;
}

__device__ __forceinline__ void norm_four(const v4f &x, double &sum, int &bad)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) norm_one(x[e], sum, bad);
}

// the elements of the quad at virtual element j that lie inside [pad, end), one by one
__device__ __forceinline__ void norm_elements(gcfloat *p, int64_t j, int pad, int64_t end, double &sum, int &bad)
{
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (j + e >= pad && j + e < end) norm_one(p[j + e - pad], sum, bad);
}

// one block of the work list: virtual elements [j0, j0 + 4096) of a tensor -> this lane's sums and counts
template <bool GRAD>
__device__ __forceinline__ void norm_block(gcfloat *w, gcfloat *grad, int64_t count, int64_t j0, int pad, bool gvec, double &sw, double &sg,
                                           int &bw, int &bg)
{
    const int tid = (int)threadIdx.x;
    const int64_t end = pad + count;                                 // virtual elements [pad, end) are the tensor
    if (j0 >= pad && j0 + SSD_UPDATE_BLOCK_ELEMS <= end && (!GRAD || gvec)) {
        // the main path: every quad of the block is inside the tensor and 16-byte aligned
        const int64_t i0 = j0 - pad + tid * 4;
        v4f x[NRM_QUADS], g[NRM_QUADS];
#pragma unroll
        for (int k = 0; k < NRM_QUADS; ++k) {
            const int64_t i = i0 + k * (NRM_THREADS * 4);
            x[k] = *(gcv4f *)(w + i);
            if (GRAD) g[k] = *(gcv4f *)(grad + i);
        }
#pragma unroll
        for (int k = 0; k < NRM_QUADS; ++k) {
            norm_four(x[k], sw, bw);
            if (GRAD) norm_four(g[k], sg, bg);
        }
    } else {
        // the block with the tensor's head or tail, or a gradient of another alignment class: whole quads where they fit and are
        // aligned, single elements otherwise -- always into the quad's own lane
#pragma unroll 1
        for (int k = 0; k < NRM_QUADS; ++k) {
            const int64_t j = j0 + (int64_t)(k * NRM_THREADS + tid) * 4;
            const bool whole = j >= pad && j + 4 <= end;
            if (whole) {
                const v4f x = *(gcv4f *)(w + (j - pad));
                norm_four(x, sw, bw);
            } else {
                norm_elements(w, j, pad, end, sw, bw);
            }
            if (GRAD) {
                if (whole && gvec) {
                    const v4f g = *(gcv4f *)(grad + (j - pad));
                    norm_four(g, sg, bg);
                } else {
                    norm_elements(grad, j, pad, end, sg, bg);
                }
            }
        }
    }
}

__global__ __launch_bounds__(NRM_THREADS) void train_norms_blocks(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                                  Partial *__restrict__ partials)
{
    __shared__ double lds_w[NRM_THREADS], lds_g[NRM_THREADS];
    __shared__ int lds_bad[NRM_THREADS];
    const int tid = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < total_blocks; c += (int)gridDim.x) {
        // the last row whose first_block <= c (a row of no blocks shares its successor's first_block and is never found)
        int lo = 0, hi = T;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tensors[mid].first_block <= c) lo = mid; else hi = mid;
        }
        const ssd_update_tensor r = tensors[lo];
        gcfloat *w = (gcfloat *)r.w, *grad = (gcfloat *)r.grad;
        const int pad = (int)(((uintptr_t)w & 15) >> 2);
        const bool gvec = (((uintptr_t)grad ^ (uintptr_t)w) & 15) == 0;
        const int64_t j0 = (int64_t)(c - r.first_block) * SSD_UPDATE_BLOCK_ELEMS;
        double sw = 0.0, sg = 0.0;
        int bw = 0, bg = 0;
        if (grad) norm_block<true>(w, grad, r.count, j0, pad, gvec, sw, sg, bw, bg);
        else norm_block<false>(w, grad, r.count, j0, pad, false, sw, sg, bw, bg);
        // the tree a[t] += a[t + s]: s = 128 and 64 through LDS, the rest inside wave 0.  A lane holds at most 16 bad elements of
        // each kind and a block 4096: both counts travel in one int
        lds_w[tid] = sw;
        lds_g[tid] = sg;
        lds_bad[tid] = bw | (bg << 16);
        __syncthreads();
        if (tid < 64) {
            sw = (lds_w[tid] + lds_w[tid + 128]) + (lds_w[tid + 64] + lds_w[tid + 192]);
            sg = (lds_g[tid] + lds_g[tid + 128]) + (lds_g[tid + 64] + lds_g[tid + 192]);
            int b = lds_bad[tid] + lds_bad[tid + 128] + lds_bad[tid + 64] + lds_bad[tid + 192];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                sw = sw + __shfl_down(sw, s, 64);
                sg = sg + __shfl_down(sg, s, 64);
                b += __shfl_down(b, s, 64);
            }
            if (tid == 0) {
                Partial p;
                p.sw = sw;
                p.sg = sg;
                p.bw = b & 0xffff;
                p.bg = b >> 16;
                partials[c] = p;
            }
        }
        __syncthreads();                                             // the next block of the stride writes the LDS again
    }
}

// stage 2, one wave per tensor: the lanes fetch 64 consecutive partials at once (one 32-byte load each, all in flight together),
// then every lane adds the 64 in ascending order, reading lane i's value with v_readlane (a constant lane: the loop is unrolled), so
// that the chain of dependent double additions is all that is serial -- the header's order; lanes past the tensor's last block hold
// +0.0, which leaves a sum that started at +0.0 and only grew by squares as it is.  The counts are integers: each lane keeps its own
// and the wave adds them at the end.  (One lane per tensor walking its blocks alone waits out a memory latency every few partials,
// and cross-lane reads through the LDS crossbar a round trip per partial: the largest tensors have 256 blocks.)
__global__ __launch_bounds__(NRM_ROW_THREADS) void train_norms_rows(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                                    const Partial *__restrict__ partials, double *__restrict__ sums,
                                                                    long long *__restrict__ bad)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = tensors[t].first_block;
    const int last = t + 1 < T ? tensors[t + 1].first_block : total_blocks;
    double sw = 0.0, sg = 0.0;
    long long bw = 0, bg = 0;
    for (int base = first; base < last; base += NRM_ROW_THREADS) {
        Partial p = {0.0, 0.0, 0, 0};
        if (base + lane < last) p = partials[base + lane];
        bw += p.bw;
        bg += p.bg;
        const int wlo = __double2loint(p.sw), whi = __double2hiint(p.sw), glo = __double2loint(p.sg), ghi = __double2hiint(p.sg);
#pragma unroll
        for (int i = 0; i < NRM_ROW_THREADS; ++i) {
            sw = sw + __hiloint2double(__builtin_amdgcn_readlane(whi, i), __builtin_amdgcn_readlane(wlo, i));
            sg = sg + __hiloint2double(__builtin_amdgcn_readlane(ghi, i), __builtin_amdgcn_readlane(glo, i));
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        bw += __shfl_xor(bw, s, 64);
        bg += __shfl_xor(bg, s, 64);
    }
    if (lane == 0) {
        sums[2 * t] = sw;
        sums[2 * t + 1] = sg;
        bad[2 * t] = bw;
        bad[2 * t + 1] = bg;
    }
}

// the TRAIN update's checks of its table (update.hip, restated: that file stays as it is), in its order and wording -> the blocks
int check_table(const char *fn, const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, int64_t *blocks_out)
{
    const std::string name(fn);
    if (!tensors_host || !tensors_dev) return ssd_fail(SSD_ERR_INVALID, name + ": bad arguments");
    if (T < 1 || T > SSD_UPDATE_MAX_TENSORS)
        return ssd_fail(SSD_ERR_INVALID, name + ": T must be in [1, " + std::to_string(SSD_UPDATE_MAX_TENSORS) + "]");
    if ((uintptr_t)tensors_dev & 7) return ssd_fail(SSD_ERR_INVALID, name + ": tensors_dev must be 8-byte aligned");
    int64_t blocks = 0;
    for (int32_t t = 0; t < T; ++t) {
        const ssd_update_tensor &d = tensors_host[t];
        const std::string row = name + ": tensor " + std::to_string(t) + ": ";
        if (d.count < 0 || d.count > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, row + "bad count");
        if (!d.w || !d.m || !d.v || !d.ema) return ssd_fail(SSD_ERR_INVALID, row + "NULL w, m, v or ema");
        if (((uintptr_t)d.w | (uintptr_t)d.m | (uintptr_t)d.v | (uintptr_t)d.ema | (uintptr_t)d.grad) & 3)
            return ssd_fail(SSD_ERR_INVALID, row + "w, m, v, ema and grad must be 4-byte aligned");
        if (d.decay != 0 && d.decay != 1) return ssd_fail(SSD_ERR_INVALID, row + "decay must be 0 or 1");
        if (d.first_block != blocks) return ssd_fail(SSD_ERR_INVALID, row + "first_block must be " + std::to_string(blocks));
        blocks += (d.count + (int64_t)(((uintptr_t)d.w >> 2) & 3) + SSD_UPDATE_BLOCK_ELEMS - 1) / SSD_UPDATE_BLOCK_ELEMS;
        if (blocks > INT_MAX) return ssd_fail(SSD_ERR_INVALID, name + ": more than 2^31 - 1 blocks");
    }
    *blocks_out = blocks;
    return SSD_OK;
}

}  // namespace

extern "C" size_t ssd_train_norms_workspace_bytes(const ssd_update_tensor *tensors_host, int32_t T)
{
    int64_t blocks = 0;
    // the planner sees no device table: any aligned non-NULL address stands in for it
    if (check_table("ssd_train_norms_workspace_bytes", tensors_host, tensors_host ? (const ssd_update_tensor *)(uintptr_t)8 : nullptr, T,
                    &blocks) != SSD_OK)
        return 0;
    return (size_t)blocks * SSD_NORMS_BLOCK_BYTES;
}

extern "C" int ssd_train_norms(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, double *sums,
                               int64_t *bad, void *workspace, size_t workspace_bytes, void *stream)
{
    int64_t blocks = 0;
    SSDCHK(check_table("ssd_train_norms", tensors_host, tensors_dev, T, &blocks));
    if (!sums || !bad) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: NULL sums or bad");
    if (((uintptr_t)sums | (uintptr_t)bad) & 7) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: sums and bad must be 8-byte aligned");
    if (!workspace) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: NULL workspace");
    if ((uintptr_t)workspace & 15) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: workspace must be 16-byte aligned");
    if (workspace_bytes < (size_t)blocks * SSD_NORMS_BLOCK_BYTES)
        return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: workspace too small: " + std::to_string(workspace_bytes) + " bytes, needs " +
                                             std::to_string((size_t)blocks * SSD_NORMS_BLOCK_BYTES));
    if (blocks > 0) {
        const unsigned grid = (unsigned)(blocks < NRM_MAX_GRID ? blocks : NRM_MAX_GRID);
        hipLaunchKernelGGL(train_norms_blocks, dim3(grid), dim3(NRM_THREADS), 0, (hipStream_t)stream, tensors_dev, (int)T, (int)blocks,
                           (Partial *)workspace);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(train_norms_rows, dim3((unsigned)T), dim3(NRM_ROW_THREADS), 0,
                       (hipStream_t)stream, tensors_dev, (int)T, (int)blocks, (const Partial *)workspace, sums, (long long *)bad);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
