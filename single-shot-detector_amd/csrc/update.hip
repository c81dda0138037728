// The TRAIN update (model.py:106-128 after the gradients): Adam with the weight-decay term's gradient, and the exponential moving
// average of every trainable variable -- every tensor of the model in one launch.  Semantics: include/ssd_hip.h, block "the TRAIN
// update".
//
//   train_update   256 lanes per block.  The work list is the model cut into blocks of SSD_UPDATE_BLOCK_ELEMS (4096) elements, each
//                  inside ONE tensor; a grid of at most TBL_MAX_GRID blocks strides over it.  A block finds its tensor by a binary
//                  search over the rows' first_block (a prefix sum the caller filled and the entry point checked): the block index is
//                  block-uniform, so the search and the row are scalar loads and every branch on the row (gradient present, decay,
//                  alignment class, whole block inside the tensor) is taken by all lanes alike.
//                  A tensor whose five addresses are congruent modulo 16 is addressed from the 16-byte boundary at or below w
//                  ("virtual" elements: the first `pad` of them lie before the tensor): a block wholly inside the tensor moves as
//                  4 x 5 16-byte loads and 4 x 4 16-byte stores per lane, all loads issued before the arithmetic; the blocks that hold
//                  the tensor's head or tail check each quad and fall to single elements where a quad crosses an end.  Any other
//                  tensor moves element by element, lane-contiguous.  Each element is read once and written once; no LDS, no atomics.
// The block shape, the row search and the types are train_table.h's; this walk reads AND writes five arrays, so it stays its own.
// Below the kernel: the host checks of an ssd_update_tensor table that train_table.h declares, for this file, train_norms.hip and
// train_hist.hip.
#include "train_table.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

static_assert(sizeof(ssd_update_scalars) == 24, "ssd_update_scalars is six floats");

struct Row {                                                        // one ssd_update_tensor, its pointers as global ones
    gfloat *w;
    const gfloat *grad;
    gfloat *m, *v, *ema;
    int64_t count;
    bool decay;
};

// steps 1-5 of include/ssd_hip.h on one element, one rounding per operation
template <bool GRAD>
__device__ __forceinline__ void update_one(float &w, float g, float &m, float &v, float &ema, bool decay, const ssd_update_scalars &s)
{
    if (GRAD) {
        if (decay) g = g + s.weight_decay * w;
        m = m + (g - m) * s.one_minus_beta1;
        v = v + (g * g - v) * s.one_minus_beta2;
        // sqrtf, not __fsqrt_rn: without fast-math it compiles to v_sqrt_f32 plus the fix-up that rounds correctly, while this
        // toolchain's __fsqrt_rn is the bare instruction (1 ulp)
        w = w - __fdiv_rn(m * s.alpha, sqrtf(v) + s.epsilon);
    }
    ema = ema - (ema - w) * s.one_minus_decay;
}

template <bool GRAD>
__device__ __forceinline__ void update_four(v4f &w, const v4f &g, v4f &m, v4f &v, v4f &ema, bool decay, const ssd_update_scalars &s)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float we = w[e], me = m[e], ve = v[e], ee = ema[e];
        update_one<GRAD>(we, g[e], me, ve, ee, decay, s);
        w[e] = we; m[e] = me; v[e] = ve; ema[e] = ee;
    }
}

template <bool GRAD>
__device__ __forceinline__ void update_scalar_at(const Row &d, int64_t i, bool decay, const ssd_update_scalars &s)
{
    float w = d.w[i], ema = d.ema[i], g = 0.0f, m = 0.0f, v = 0.0f;
    if (GRAD) {
        g = d.grad[i];
        m = d.m[i];
        v = d.v[i];
    }
    update_one<GRAD>(w, g, m, v, ema, decay, s);
    if (GRAD) {
        d.w[i] = w;
        d.m[i] = m;
        d.v[i] = v;
    }
    d.ema[i] = ema;
}

template <bool GRAD>
__device__ __forceinline__ void update_quad_at(const Row &d, int64_t i, bool decay, const ssd_update_scalars &s)
{
    // i: element index of a quad whose five addresses are 16-byte aligned and which lies wholly inside the tensor
    v4f w = *(const gv4f *)(d.w + i), ema = *(const gv4f *)(d.ema + i), g = v4f{0, 0, 0, 0}, m = g, v = g;
    if (GRAD) {
        g = *(const gv4f *)(d.grad + i);
        m = *(const gv4f *)(d.m + i);
        v = *(const gv4f *)(d.v + i);
    }
    update_four<GRAD>(w, g, m, v, ema, decay, s);
    if (GRAD) {
        *(gv4f *)(d.w + i) = w;
        *(gv4f *)(d.m + i) = m;
        *(gv4f *)(d.v + i) = v;
    }
    *(gv4f *)(d.ema + i) = ema;
}

// one block of the work list: virtual elements [j0, j0 + 4096) of tensor d
template <bool GRAD>
__device__ __forceinline__ void update_block(const Row &d, int64_t j0, int pad, bool vec, const ssd_update_scalars &s)
{
    const bool decay = d.decay;
    const int tid = (int)threadIdx.x;
    const int64_t end = pad + d.count;                               // virtual elements [pad, end) are the tensor
    if (vec && j0 >= pad && j0 + SSD_UPDATE_BLOCK_ELEMS <= end) {
        // the main path: every quad of the block is inside the tensor
        const int64_t i0 = j0 - pad + tid * 4;
        v4f w[TBL_QUADS], ema[TBL_QUADS], g[TBL_QUADS], m[TBL_QUADS], v[TBL_QUADS];
#pragma unroll
        for (int k = 0; k < TBL_QUADS; ++k) {
            const int64_t i = i0 + k * TBL_STEP;
            w[k] = *(const gv4f *)(d.w + i);
            ema[k] = *(const gv4f *)(d.ema + i);
            if (GRAD) {
                g[k] = *(const gv4f *)(d.grad + i);
                m[k] = *(const gv4f *)(d.m + i);
                v[k] = *(const gv4f *)(d.v + i);
            } else {
                g[k] = m[k] = v[k] = v4f{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int k = 0; k < TBL_QUADS; ++k) {
            const int64_t i = i0 + k * TBL_STEP;
            update_four<GRAD>(w[k], g[k], m[k], v[k], ema[k], decay, s);
            if (GRAD) {
                *(gv4f *)(d.w + i) = w[k];
                *(gv4f *)(d.m + i) = m[k];
                *(gv4f *)(d.v + i) = v[k];
            }
            *(gv4f *)(d.ema + i) = ema[k];
        }
    } else if (vec) {
        // the block with the tensor's head or tail: whole quads where they fit, single elements where a quad crosses an end
#pragma unroll 1
        for (int k = 0; k < TBL_QUADS; ++k) {
            const int64_t j = j0 + (int64_t)(k * TBL_THREADS + tid) * 4;
            if (j >= pad && j + 4 <= end) {
                update_quad_at<GRAD>(d, j - pad, decay, s);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (j + e >= pad && j + e < end) update_scalar_at<GRAD>(d, j + e - pad, decay, s);
            }
        }
    } else {
        // addresses of different alignment classes (pad == 0 here): element by element, consecutive lanes on consecutive elements
#pragma unroll 1
        for (int k = 0; k < TBL_QUADS * 4; ++k) {
            const int64_t j = j0 + k * TBL_THREADS + tid;
            if (j < end) update_scalar_at<GRAD>(d, j, decay, s);
        }
    }
}

__global__ __launch_bounds__(TBL_THREADS) void train_update(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                            ssd_update_scalars s)
{
    for (int c = (int)blockIdx.x; c < total_blocks; c += (int)gridDim.x) {
        const ssd_update_tensor r = tensors[row_of_block(tensors, T, &ssd_update_tensor::first_block, c)];
        const Row d = {(gfloat *)r.w, (const gfloat *)r.grad, (gfloat *)r.m, (gfloat *)r.v, (gfloat *)r.ema, r.count, r.decay != 0};
        const uintptr_t a = (uintptr_t)d.w & 15;
        const bool vec = ((uintptr_t)d.m & 15) == a && ((uintptr_t)d.v & 15) == a && ((uintptr_t)d.ema & 15) == a &&
                         (!d.grad || ((uintptr_t)d.grad & 15) == a);
        const int pad = vec ? (int)(a >> 2) : 0;
        const int64_t j0 = (int64_t)(c - r.first_block) * SSD_UPDATE_BLOCK_ELEMS;
        if (d.grad) update_block<true>(d, j0, pad, vec, s);
        else update_block<false>(d, j0, pad, vec, s);
    }
}

}  // namespace

// ----------------------------------------------------------------------------- the table's host checks (train_table.h)
int check_update_args(const char *fn, const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, bool others)
{
    const std::string name(fn);
    if (!tensors_host || !tensors_dev || !others) return ssd_fail(SSD_ERR_INVALID, name + ": bad arguments");
    if (T < 1 || T > SSD_UPDATE_MAX_TENSORS)
        return ssd_fail(SSD_ERR_INVALID, name + ": T must be in [1, " + std::to_string(SSD_UPDATE_MAX_TENSORS) + "]");
    if ((uintptr_t)tensors_dev & 7) return ssd_fail(SSD_ERR_INVALID, name + ": tensors_dev must be 8-byte aligned");
    return SSD_OK;
}

int check_update_rows(const char *fn, const ssd_update_tensor *tensors_host, int32_t T, int64_t *blocks_out)
{
    const std::string name(fn);
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

int check_update_table(const char *fn, const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, int64_t *blocks_out)
{
    SSDCHK(check_update_args(fn, tensors_host, tensors_dev, T));
    return check_update_rows(fn, tensors_host, T, blocks_out);
}

size_t update_table_bytes(const char *fn, const ssd_update_tensor *tensors_host, int32_t T, size_t block_bytes)
{
    int64_t blocks = 0;
    // the planner sees no device table: any aligned non-NULL address stands in for it
    if (check_update_table(fn, tensors_host, (const ssd_update_tensor *)(uintptr_t)8, T, &blocks) != SSD_OK) return 0;
    return (size_t)blocks * block_bytes;
}

int check_workspace(const char *fn, const void *workspace, size_t workspace_bytes, size_t needs)
{
    const std::string name(fn);
    if (!workspace) return ssd_fail(SSD_ERR_INVALID, name + ": NULL workspace");
    if ((uintptr_t)workspace & 15) return ssd_fail(SSD_ERR_INVALID, name + ": workspace must be 16-byte aligned");
    if (workspace_bytes < needs)
        return ssd_fail(SSD_ERR_INVALID, name + ": workspace too small: " + std::to_string(workspace_bytes) + " bytes, needs " + std::to_string(needs));
    return SSD_OK;
}

extern "C" int ssd_train_update(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T,
                                const ssd_update_scalars *scalars, void *stream)
{
    SSDCHK(check_update_args("ssd_train_update", tensors_host, tensors_dev, T, scalars != nullptr));
    const float sc[6] = {scalars->alpha, scalars->one_minus_beta1, scalars->one_minus_beta2, scalars->epsilon, scalars->weight_decay,
                         scalars->one_minus_decay};
    for (float x : sc)
        if (!std::isfinite(x)) return ssd_fail(SSD_ERR_INVALID, "ssd_train_update: non-finite scalar");
    int64_t blocks = 0;
    SSDCHK(check_update_rows("ssd_train_update", tensors_host, T, &blocks));
    if (blocks == 0) return SSD_OK;                                   // every tensor is empty
    hipLaunchKernelGGL(train_update, dim3(grid_for(blocks)), dim3(TBL_THREADS), 0, (hipStream_t)stream, tensors_dev, (int)T, (int)blocks, *scalars);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
