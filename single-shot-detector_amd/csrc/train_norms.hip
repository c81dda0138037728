// The TRAIN step's norms: sum w^2, sum g^2 and the non-finite counts of every tensor of the update's table, before the update
// consumes the gradients.  Semantics and the ORDER of the double additions: include/ssd_hip.h, block "the TRAIN step's norms".
//
//   train_norms_blocks   stage 1 over the update's work list (train_table.h: the block shape, the row search, walk_block): a lane
//                        squares its 16 elements of w, and of grad where there is one, in double, quad by quad; the 256 lane values
//                        go through tree256.  Lane 0 writes the block's 32-byte partial with two 16-byte vector stores.
//   train_norms_rows     stage 2: one wave per tensor loads 64 of its blocks' partials at a time and adds them in ascending block
//                        order (wave_ordered_add).
// No atomics; reads w and grad, writes the workspace and the outputs only.
#include "train_table.h"

#pragma clang fp contract(off)

namespace {

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

__global__ __launch_bounds__(TBL_THREADS) void train_norms_blocks(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                                  Partial *__restrict__ partials)
{
    __shared__ double lds_d[2][TBL_THREADS];
    __shared__ int lds_bad[TBL_THREADS];
    const int tid = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < total_blocks; c += (int)gridDim.x) {
        const ssd_update_tensor r = tensors[row_of_block(tensors, T, &ssd_update_tensor::first_block, c)];
        const gfloat *w = (const gfloat *)r.w, *grad = (const gfloat *)r.grad;
        const int pad = (int)(((uintptr_t)w & 15) >> 2);
        const bool gvec = (((uintptr_t)grad ^ (uintptr_t)w) & 15) == 0;
        const int64_t j0 = (int64_t)(c - r.first_block) * SSD_UPDATE_BLOCK_ELEMS;
        double s[2] = {0.0, 0.0};                                    // w, grad
        int bw = 0, bg = 0;
        // `in` is not looked at: an element outside the tensor arrives as a finite +0.0f, which adds +0.0 to a sum that started at
        // +0.0 and only ever grew by squares -- no bit of it moves -- and 0 to the count
        if (grad) walk_block<true>(w, grad, r.count, j0, pad, gvec, [&](float x, float g, bool) { norm_one(x, s[0], bw); norm_one(g, s[1], bg); });
        else walk_block<false>(w, grad, r.count, j0, pad, false, [&](float x, float, bool) { norm_one(x, s[0], bw); });
        // a lane holds at most 16 bad elements of each kind and a block 4096: both counts travel in one int, added in any order
        lds_bad[tid] = bw | (bg << 16);
        tree256<2>(s, lds_d);
        if (tid < 64) {
            int b = lds_bad[tid] + lds_bad[tid + 128] + lds_bad[tid + 64] + lds_bad[tid + 192];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) b += __shfl_down(b, m, 64);
            if (tid == 0) {
                Partial p;
                p.sw = s[0];
                p.sg = s[1];
                p.bw = b & 0xffff;
                p.bg = b >> 16;
                partials[c] = p;
            }
        }
        __syncthreads();                                             // the next block of the stride writes the LDS again
    }
}

// stage 2, one wave per tensor.  The counts are integers: each lane keeps its own and the wave adds them at the end.
__global__ __launch_bounds__(TBL_WAVE) void train_norms_rows(const ssd_update_tensor *__restrict__ tensors, int T, int total_blocks,
                                                             const Partial *__restrict__ partials, double *__restrict__ sums,
                                                             long long *__restrict__ bad)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = tensors[t].first_block;
    const int last = t + 1 < T ? tensors[t + 1].first_block : total_blocks;
    double s[2] = {0.0, 0.0};
    long long bw = 0, bg = 0;
    for (int base = first; base < last; base += TBL_WAVE) {
        Partial p = {0.0, 0.0, 0, 0};
        if (base + lane < last) p = partials[base + lane];
        bw += p.bw;
        bg += p.bg;
        const double v[2] = {p.sw, p.sg};
        wave_ordered_add<2>(s, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        bw += __shfl_xor(bw, m, 64);
        bg += __shfl_xor(bg, m, 64);
    }
    if (lane == 0) {
        sums[2 * t] = s[0];
        sums[2 * t + 1] = s[1];
        bad[2 * t] = bw;
        bad[2 * t + 1] = bg;
    }
}

}  // namespace

extern "C" size_t ssd_train_norms_workspace_bytes(const ssd_update_tensor *tensors_host, int32_t T)
{
    return update_table_bytes("ssd_train_norms_workspace_bytes", tensors_host, T, SSD_NORMS_BLOCK_BYTES);
}

extern "C" int ssd_train_norms(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, double *sums,
                               int64_t *bad, void *workspace, size_t workspace_bytes, void *stream)
{
    int64_t blocks = 0;
    SSDCHK(check_update_table("ssd_train_norms", tensors_host, tensors_dev, T, &blocks));
    if (!sums || !bad) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: NULL sums or bad");
    if (((uintptr_t)sums | (uintptr_t)bad) & 7) return ssd_fail(SSD_ERR_INVALID, "ssd_train_norms: sums and bad must be 8-byte aligned");
    SSDCHK(check_workspace("ssd_train_norms", workspace, workspace_bytes, (size_t)blocks * SSD_NORMS_BLOCK_BYTES));
    if (blocks > 0) {
        hipLaunchKernelGGL(train_norms_blocks, dim3(grid_for(blocks)), dim3(TBL_THREADS), 0, (hipStream_t)stream, tensors_dev, (int)T,
                           (int)blocks, (Partial *)workspace);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(train_norms_rows, dim3((unsigned)T), dim3(TBL_WAVE), 0, (hipStream_t)stream, tensors_dev, (int)T, (int)blocks,
                       (const Partial *)workspace, sums, (long long *)bad);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
