// The TRAIN step's gradient exchange: one slice per rank packed for ONE all-gather, the gathered slices summed in ascending rank
// order.  Semantics, the bucket layout and every refusal: include/ssd_hip.h, block "the TRAIN step's gradient exchange".
//
//   walk_rows      under both kernels.  256 lanes per block; the work list is the payload cut into blocks of SSD_UPDATE_BLOCK_ELEMS
//                  (4096) bucket floats; a grid of at most TBL_MAX_GRID blocks strides over it (train_table.h: the shape, the row
//                  search).  A block finds the row that holds its first float by the search over the rows' offset (block-uniform:
//                  scalar loads, every branch on a row taken by all lanes alike) and walks the rows from there until one starts
//                  behind the block.
//   grad_pack      Offsets are multiples of 4 and the payload is 16-byte aligned, so a bucket quad lies inside ONE row and is
//                  always stored as 16 bytes; it is loaded
//                  as 16 bytes where the row's data is 16-byte aligned and the quad lies inside the tensor, else element by element
//                  (+0.0 behind the tensor's end and for a NULL row).  A block wholly inside one aligned tensor -- nearly all of a
//                  model's floats -- moves as 4 loads then 4 stores per lane.  Block 0 also writes the 16 header floats.
//   grad_reduce<G> the same work list over the gathered buffer.  c_r is computed once per block, before the stride loop; a lane
//                  issues the G loads of a quad (one per slice) before the arithmetic, adds in ascending rank order and stores to
//                  the row's data as 16 bytes, or element by element where data is not 16-byte aligned or the quad crosses the
//                  tensor's end.  G is a template parameter (1 .. SSD_REDUCE_MAX_RANKS): the slices' quads and the c_r stay in
//                  registers.  Block 0's lane 0 writes losses_out and weights_out.  No LDS, no atomics.
#include "train_table.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int64_t RED_BLOCK = SSD_UPDATE_BLOCK_ELEMS;
static_assert(sizeof(ssd_reduce_row) == 32, "ssd_reduce_row is the 32-byte row of include/ssd_hip.h");
static_assert(offsetof(ssd_reduce_row, count) == 8 && offsetof(ssd_reduce_row, offset) == 16 && offsetof(ssd_reduce_row, kind) == 24,
              "ssd_reduce_row has no padding");
static_assert(SSD_REDUCE_HEADER_FLOATS % 4 == 0, "the payload starts on a 16-byte boundary of the slice");

__device__ __forceinline__ int64_t roundup4(int64_t n) { return (n + 3) & ~(int64_t)3; }

__device__ __forceinline__ float at_least_one(float a) { return a > 1.0f ? a : 1.0f; }

// One block of the work list, bucket floats [b0, b0 + 4096): every row with floats in it, from the row of b0 on (of rows that share
// an offset -- empty ones -- the search finds the last), empty rows skipped and, with NEED_DATA, rows whose data is NULL.  A block
// wholly inside one 16-byte aligned tensor is main(r, data); of any other row, this lane's quads j inside the block are
// quad(r, data, vec, j), vec: data is there and 16-byte aligned.
template <bool NEED_DATA, class Main, class Quad>
__device__ __forceinline__ void walk_rows(const ssd_reduce_row *__restrict__ rows, int T, int64_t b0, Main main, Quad quad)
{
    const int64_t b1 = b0 + RED_BLOCK;
    for (int t = row_of_block(rows, T, &ssd_reduce_row::offset, b0); t < T; ++t) {
        const ssd_reduce_row r = rows[t];
        if (r.offset >= b1) break;
        gfloat *data = (gfloat *)r.data;
        if (NEED_DATA && !data) continue;
        const int64_t s0 = r.offset > b0 ? r.offset : b0;
        const int64_t rend = r.offset + roundup4(r.count), s1 = rend < b1 ? rend : b1;
        if (s1 <= s0) continue;                                      // an empty row
        const bool vec = data && ((uintptr_t)data & 15) == 0;
        if (vec && s0 == b0 && r.offset + r.count >= b1) {
            main(r, data);                                           // the main path: 4 quads per lane, unrolled
        } else {
#pragma unroll 1
            for (int64_t j = s0 + (int)threadIdx.x * 4; j < s1; j += TBL_STEP) quad(r, data, vec, j);
        }
    }
}

// ----------------------------------------------------------------------------- pack
__global__ __launch_bounds__(TBL_THREADS) void grad_pack(const ssd_reduce_row *__restrict__ rows, int T, int64_t used, int blocks,
                                                         const gfloat *__restrict__ header, gfloat *__restrict__ slice)
{
    const int tid = (int)threadIdx.x;
    if (blockIdx.x == 0 && tid < SSD_REDUCE_HEADER_FLOATS) slice[tid] = tid < 3 ? header[tid] : 0.0f;
    gfloat *pay = slice + SSD_REDUCE_HEADER_FLOATS;
    for (int c = (int)blockIdx.x; c < blocks; c += (int)gridDim.x) {
        const int64_t b0 = (int64_t)c * RED_BLOCK, b1 = b0 + RED_BLOCK;
        walk_rows<false>(
            rows, T, b0,
            [&](const ssd_reduce_row &r, const gfloat *data) {
                const int64_t j0 = b0 + tid * 4;
                v4f x[TBL_QUADS];
#pragma unroll
                for (int k = 0; k < TBL_QUADS; ++k) x[k] = *(const gv4f *)(data + (j0 + k * TBL_STEP - r.offset));
#pragma unroll
                for (int k = 0; k < TBL_QUADS; ++k) *(gv4f *)(pay + j0 + k * TBL_STEP) = x[k];
            },
            [&](const ssd_reduce_row &r, const gfloat *data, bool vec, int64_t j) {
                const int64_t i = j - r.offset;                      // the quad's first element
                v4f x = v4f{0, 0, 0, 0};
                if (vec && i + 4 <= r.count) {
                    x = *(const gv4f *)(data + i);
                } else if (data) {
                    for (int e = 0; e < 4; ++e)
                        if (i + e < r.count) x[e] = data[i + e];
                }
                *(gv4f *)(pay + j) = x;
            });
        if (used < b1) {                                             // the payload behind the last row
#pragma unroll 1
            for (int64_t j = (used > b0 ? used : b0) + tid * 4; j < b1; j += TBL_STEP) *(gv4f *)(pay + j) = v4f{0, 0, 0, 0};
        }
    }
}

// ----------------------------------------------------------------------------- reduce
// the header's rule on one element of every slice, x[r] of rank r
template <int G>
__device__ __forceinline__ float reduce_one(const float (&x)[G], const float (&c)[G], bool mean, float inv_g)
{
    if (mean) {
        float acc = x[0];
#pragma unroll
        for (int r = 1; r < G; ++r) acc = acc + x[r];
        return acc * inv_g;
    }
    float acc = x[0] * c[0];
#pragma unroll
    for (int r = 1; r < G; ++r) acc = acc + x[r] * c[r];
    return acc;
}

template <int G>
__device__ __forceinline__ v4f reduce_four(const v4f (&x)[G], const float (&c)[G], bool mean, float inv_g)
{
    v4f out;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float xe[G];
#pragma unroll
        for (int r = 0; r < G; ++r) xe[r] = x[r][e];
        out[e] = reduce_one<G>(xe, c, mean, inv_g);
    }
    return out;
}

template <int G>
__global__ __launch_bounds__(TBL_THREADS) void grad_reduce(const ssd_reduce_row *__restrict__ rows, int T, int blocks,
                                                           const gfloat *__restrict__ gathered, int64_t slice_floats,
                                                           gfloat *__restrict__ losses_out, gfloat *__restrict__ weights_out)
{
    const int tid = (int)threadIdx.x;
    // once per block: the ranks' weights from the G headers
    float n[G], c[G];
#pragma unroll
    for (int r = 0; r < G; ++r) n[r] = gathered[r * slice_floats];
    float S = n[0];
#pragma unroll
    for (int r = 1; r < G; ++r) S = S + n[r];
    const float D = at_least_one(S);
#pragma unroll
    for (int r = 0; r < G; ++r) c[r] = __fdiv_rn(at_least_one(n[r]), D);
    const float inv_g = __fdiv_rn(1.0f, (float)G);
    if (blockIdx.x == 0 && tid == 0) {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float x[G];
#pragma unroll
            for (int r = 0; r < G; ++r) x[r] = gathered[r * slice_floats + 1 + w];
            losses_out[w] = reduce_one<G>(x, c, false, inv_g);
        }
#pragma unroll
        for (int r = 0; r < G; ++r) weights_out[r] = c[r];
    }
    const gfloat *pay = gathered + SSD_REDUCE_HEADER_FLOATS;
    for (int cb = (int)blockIdx.x; cb < blocks; cb += (int)gridDim.x) {
        const int64_t b0 = (int64_t)cb * RED_BLOCK;
        walk_rows<true>(                                             // a row without data: nothing goes back
            rows, T, b0,
            [&](const ssd_reduce_row &r, gfloat *data) {
                const int64_t j0 = b0 + tid * 4;
#pragma unroll
                for (int k = 0; k < TBL_QUADS; ++k) {
                    const int64_t j = j0 + k * TBL_STEP;
                    v4f x[G];
#pragma unroll
                    for (int q = 0; q < G; ++q) x[q] = *(const gv4f *)(pay + q * slice_floats + j);
                    *(gv4f *)(data + (j - r.offset)) = reduce_four<G>(x, c, r.kind != 0, inv_g);
                }
            },
            [&](const ssd_reduce_row &r, gfloat *data, bool vec, int64_t j) {
                const int64_t i = j - r.offset;                      // the quad's first element
                v4f x[G];
#pragma unroll
                for (int q = 0; q < G; ++q) x[q] = *(const gv4f *)(pay + q * slice_floats + j);
                const v4f y = reduce_four<G>(x, c, r.kind != 0, inv_g);
                if (vec && i + 4 <= r.count) {
                    *(gv4f *)(data + i) = y;
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (i + e < r.count) data[i + e] = y[e];
                }
            });
    }
}

template <int G>
void launch_reduce(unsigned grid, hipStream_t s, const ssd_reduce_row *rows, int T, int blocks, const float *gathered,
                   int64_t slice_floats, float *losses_out, float *weights_out)
{
    hipLaunchKernelGGL(grad_reduce<G>, dim3(grid), dim3(TBL_THREADS), 0, s, rows, T, blocks, (const gfloat *)gathered, slice_floats,
                       (gfloat *)losses_out, (gfloat *)weights_out);
}

// the table's refusals, shared by the three entry points -> SSD_OK and the payload floats in use (`used`) and in all (`P`)
int check_rows(const std::string &who, const ssd_reduce_row *rows_host, int32_t T, int64_t &used, int64_t &P)
{
    if (!rows_host) return ssd_fail(SSD_ERR_INVALID, who + ": bad arguments");
    if (T < 1 || T > SSD_UPDATE_MAX_TENSORS)
        return ssd_fail(SSD_ERR_INVALID, who + ": T must be in [1, " + std::to_string(SSD_UPDATE_MAX_TENSORS) + "]");
    int64_t offset = 0;
    std::vector<std::pair<uintptr_t, uintptr_t>> spans;
    for (int32_t t = 0; t < T; ++t) {
        const ssd_reduce_row &d = rows_host[t];
        const std::string row = who + ": row " + std::to_string(t) + ": ";
        if (d.count < 0 || d.count > ((int64_t)1 << 40)) return ssd_fail(SSD_ERR_INVALID, row + "bad count");
        if ((uintptr_t)d.data & 3) return ssd_fail(SSD_ERR_INVALID, row + "data must be 4-byte aligned");
        if (d.kind != 0 && d.kind != 1) return ssd_fail(SSD_ERR_INVALID, row + "kind must be 0 or 1");
        if (d.offset != offset) return ssd_fail(SSD_ERR_INVALID, row + "offset must be " + std::to_string(offset));
        offset += (d.count + 3) / 4 * 4;
        if (d.data && d.count > 0) spans.emplace_back((uintptr_t)d.data, (uintptr_t)d.data + 4 * (uintptr_t)d.count);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k].first < spans[k - 1].second) return ssd_fail(SSD_ERR_INVALID, who + ": the rows' data ranges overlap");
    used = offset;
    P = (offset + RED_BLOCK - 1) / RED_BLOCK * RED_BLOCK;
    if (P / RED_BLOCK > INT_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": more than 2^31 - 1 blocks");
    return SSD_OK;
}

}  // namespace

extern "C" int64_t ssd_train_bucket_floats(const ssd_reduce_row *rows_host, int32_t T)
{
    int64_t used = 0, P = 0;
    if (check_rows("ssd_train_bucket_floats", rows_host, T, used, P) != SSD_OK) return 0;
    return SSD_REDUCE_HEADER_FLOATS + P;
}

extern "C" int ssd_train_grad_pack(const ssd_reduce_row *rows_host, const ssd_reduce_row *rows_dev, int32_t T, const float *header_dev,
                                   float *slice, int64_t slice_floats, void *stream)
{
    const std::string who = "ssd_train_grad_pack";
    if (!rows_host || !rows_dev || !header_dev || !slice) return ssd_fail(SSD_ERR_INVALID, who + ": bad arguments");
    if ((uintptr_t)rows_dev & 7) return ssd_fail(SSD_ERR_INVALID, who + ": rows_dev must be 8-byte aligned");
    if ((uintptr_t)header_dev & 3) return ssd_fail(SSD_ERR_INVALID, who + ": header_dev must be 4-byte aligned");
    if ((uintptr_t)slice & 15) return ssd_fail(SSD_ERR_INVALID, who + ": slice must be 16-byte aligned");
    int64_t used = 0, P = 0;
    SSDCHK(check_rows(who, rows_host, T, used, P));
    if (slice_floats != SSD_REDUCE_HEADER_FLOATS + P)
        return ssd_fail(SSD_ERR_INVALID, who + ": slice_floats must be " + std::to_string(SSD_REDUCE_HEADER_FLOATS + P));
    const int64_t blocks = P / RED_BLOCK;
    const unsigned grid = grid_for(blocks < 1 ? 1 : blocks);          // block 0: the header
    hipLaunchKernelGGL(grad_pack, dim3(grid), dim3(TBL_THREADS), 0, (hipStream_t)stream, rows_dev, (int)T, used, (int)blocks,
                       (const gfloat *)header_dev, (gfloat *)slice);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

extern "C" int ssd_train_grad_reduce(const ssd_reduce_row *rows_host, const ssd_reduce_row *rows_dev, int32_t T, const float *gathered,
                                     int32_t G, int64_t slice_floats, float *losses_out, float *weights_out, void *stream)
{
    const std::string who = "ssd_train_grad_reduce";
    if (!rows_host || !rows_dev || !gathered || !losses_out || !weights_out) return ssd_fail(SSD_ERR_INVALID, who + ": bad arguments");
    if ((uintptr_t)rows_dev & 7) return ssd_fail(SSD_ERR_INVALID, who + ": rows_dev must be 8-byte aligned");
    if ((uintptr_t)gathered & 15) return ssd_fail(SSD_ERR_INVALID, who + ": gathered must be 16-byte aligned");
    if (((uintptr_t)losses_out | (uintptr_t)weights_out) & 3)
        return ssd_fail(SSD_ERR_INVALID, who + ": losses_out and weights_out must be 4-byte aligned");
    if (G < 1 || G > SSD_REDUCE_MAX_RANKS)
        return ssd_fail(SSD_ERR_INVALID, who + ": G must be in [1, " + std::to_string(SSD_REDUCE_MAX_RANKS) + "]");
    int64_t used = 0, P = 0;
    SSDCHK(check_rows(who, rows_host, T, used, P));
    if (slice_floats != SSD_REDUCE_HEADER_FLOATS + P)
        return ssd_fail(SSD_ERR_INVALID, who + ": slice_floats must be " + std::to_string(SSD_REDUCE_HEADER_FLOATS + P));
    const int64_t blocks = P / RED_BLOCK;
    const unsigned grid = grid_for(blocks < 1 ? 1 : blocks);          // block 0: losses, weights
    const hipStream_t s = (hipStream_t)stream;
    switch (G) {
#define RED_CASE(g) case g: launch_reduce<g>(grid, s, rows_dev, (int)T, (int)blocks, gathered, slice_floats, losses_out, weights_out); break;
        RED_CASE(1) RED_CASE(2) RED_CASE(3) RED_CASE(4) RED_CASE(5) RED_CASE(6) RED_CASE(7) RED_CASE(8)
        RED_CASE(9) RED_CASE(10) RED_CASE(11) RED_CASE(12) RED_CASE(13) RED_CASE(14) RED_CASE(15) RED_CASE(16)
#undef RED_CASE
    }
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
