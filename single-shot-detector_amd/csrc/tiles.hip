// Tiled detection: frames larger than the network's input as overlapping tiles of the network's own size, and the merge of the
// tiles' records (and the whole frame's) by the detector's NMS rule.  The grid, the merge's semantics and every refusal:
// include/ssd_hip.h, block "tiled detection".
//
//   tile_gather  a streaming copy, one lane per 16 output bytes (a tile row is 3 * tw bytes = a multiple of 384: whole groups), a
//                grid-strided loop over the groups of all tiles.  The source row starts at any byte, so a lane fetches the four or
//                five 4-byte ALIGNED dwords that cover its 16 bytes through a buffer resource of exactly the frame block's size and
//                funnels neighbours (v_alignbyte).  A dword load is issued only when its four bytes lie inside the block; the at most
//                two dwords that straddle the block's ends are put together from single-byte loads, of which the resource drops the
//                ones outside.  No LDS.
//   tile_select  one wave per (frame, class).  The wave walks the frame's sources in order (its tiles, then the whole frame's
//                record) and compacts the rows of its class into LDS in order (ballot + popcount: the position IS the candidate
//                index), moving a tile's boxes to frame coordinates on the way.  Then at most m rounds of {wave arg-max of
//                (score, lowest index) over the live candidates -> keep -> every lane drops its live candidates whose IoU with the
//                kept box is > iou_threshold}: the arg-max of the survivors is the next box greedy NMS keeps (postprocess.hip K9c).
//                The kept rows go to the output record's own rows c * m .., the unused ones of the m get label -1.
//   tile_pack    one block per frame closes the gaps IN PLACE: chunks of 256 rows in ascending order, every row read into
//                registers before the barrier of the chunk's prefix sum, written behind it to a row that is never above its own
//                (so never one a later chunk still has to read); then zeros from num_boxes on, and num_boxes.
// No atomics anywhere.
#include "host.h"
#include "iou_greater.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_a4 __attribute__((aligned(4)));

constexpr int TG_THREADS = 256;
constexpr int TG_GRID_CAP = 8192;
constexpr int TM_CAP = SSD_TILE_MAX_CANDIDATES;
constexpr int TM_PER_LANE = TM_CAP / 64;
static_assert(TM_CAP % 64 == 0 && TM_PER_LANE <= 32, "a lane's live candidates are the bits of one 32-bit mask");
static_assert(TM_CAP >= 1024, "the documented floor of the cap");

struct TileGrid { int ny, nx, sy, sx; };

__device__ __forceinline__ int tile_origin(int i, int step, int last) { return min(i * step, last); }

// the dword at byte offset `a` of the block (the ADDRESS is 4-byte aligned, `a` itself may be -3 .. -1 or end within 3 bytes of n):
// bytes outside [0, n) read as 0 and are never fetched
__device__ __forceinline__ unsigned block_dword(const __amdgpu_buffer_rsrc_t rsrc, int a, int n)
{
    if (a >= 0 && a <= n - 4) return __builtin_amdgcn_raw_buffer_load_b32(rsrc, a, 0, 0);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = a + j;
        // (an offset outside the block, a negative one included, is past the resource's bound: the load returns 0)
        v |= (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsrc, (o >= 0 && o < n) ? o : (int)0x80000000u, 0, 0) << (8 * j);
    }
    return v;
}

__global__ __launch_bounds__(TG_THREADS) void tile_gather(const uint8_t *__restrict__ frames, int nbytes, int H, int W, int th, int tw,
                                                          TileGrid g, long long groups, int row_groups, uint8_t *__restrict__ tiles)
{
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)frames, 0, nbytes, 0x00020000);
    const int skew = (int)((uintptr_t)frames & 3);
    const long long stride = (long long)gridDim.x * TG_THREADS;
    for (long long q = (long long)blockIdx.x * TG_THREADS + threadIdx.x; q < groups; q += stride) {
        const long long r = q / row_groups;                 // row of the tile block: t * th + y
        const int c = (int)(q - r * row_groups);
        const long long t = r / th;
        const int y = (int)(r - t * th);
        const long long u = t / g.nx;
        const int ix = (int)(t - u * g.nx);
        const int f = (int)(u / g.ny);
        const int iy = (int)(u - (long long)f * g.ny);
        const int y0 = tile_origin(iy, g.sy, H - th), x0 = tile_origin(ix, g.sx, W - tw);
        const int s = ((f * H + y0 + y) * W + x0) * 3 + c * 16;     // < nbytes < 2^31 (host check)
        const int mis = (skew + s) & 3;
        const int a = s - mis;                              // frames + a is 4-byte aligned; a >= -3
        v4u d;
        if (a >= 0 && a <= nbytes - 16) {
            d = __builtin_amdgcn_raw_buffer_load_b128(rsrc, a, 0, 0);
        } else {
            d[0] = block_dword(rsrc, a, nbytes);
            d[1] = block_dword(rsrc, a + 4, nbytes);
            d[2] = block_dword(rsrc, a + 8, nbytes);
            d[3] = block_dword(rsrc, a + 12, nbytes);
        }
        const unsigned d4 = mis ? block_dword(rsrc, a + 16, nbytes) : 0u;
        v4u o;
        o[0] = __builtin_amdgcn_alignbyte(d[1], d[0], mis);
        o[1] = __builtin_amdgcn_alignbyte(d[2], d[1], mis);
        o[2] = __builtin_amdgcn_alignbyte(d[3], d[2], mis);
        o[3] = __builtin_amdgcn_alignbyte(d4, d[3], mis);
        *(v4u_a4 *)(tiles + q * 16) = o;
    }
}

struct MergeArgs {
    const int *tiles, *full;
    int *out;
    int H, W, th, tw;
    TileGrid g;
    int C, m, T;
    float thr;
};

// float bits -> an unsigned that orders like the float (-0 with +0, as the comparison of floats has it)
__device__ __forceinline__ unsigned score_order(unsigned bits)
{
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}

__global__ __launch_bounds__(64) void tile_select(const MergeArgs p)
{
    __shared__ v4f s_box[TM_CAP];
    __shared__ unsigned s_score[TM_CAP];
    const int lane = (int)threadIdx.x;
    const int f = (int)blockIdx.x / p.C, c = (int)blockIdx.x - f * p.C;
    const int T = p.T, nt = p.g.ny * p.g.nx, nsrc = nt + (p.full ? 1 : 0);
    const long long words = 6ll * T + 1;
    const unsigned long long below = (1ull << lane) - 1ull;

    // ---- the candidates, in order
    int n = 0;
    for (int s = 0; s < nsrc; ++s) {
        const bool tile = s < nt;
        const int *rec = tile ? p.tiles + ((long long)f * nt + s) * words : p.full + (long long)f * words;
        int nb = rec[6ll * T];
        nb = nb < 0 ? 0 : (nb > T ? T : nb);
        const int iy = s / p.g.nx, ix = s - iy * p.g.nx;
        const float y0 = (float)tile_origin(iy, p.g.sy, p.H - p.th), x0 = (float)tile_origin(ix, p.g.sx, p.W - p.tw);
        const float fth = (float)p.th, ftw = (float)p.tw, fH = (float)p.H, fW = (float)p.W;
        for (int base = 0; base < nb; base += 64) {
            const int row = base + lane;
            const bool hit = row < nb && rec[5ll * T + row] == c;
            const unsigned long long votes = __ballot(hit);
            const int pos = n + __popcll(votes & below);
            if (hit && pos < TM_CAP) {
                v4f b;
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = __int_as_float(rec[4ll * row + k]);
                if (tile) {
                    b[0] = __fdiv_rn(__fadd_rn(__fmul_rn(b[0], fth), y0), fH);
                    b[1] = __fdiv_rn(__fadd_rn(__fmul_rn(b[1], ftw), x0), fW);
                    b[2] = __fdiv_rn(__fadd_rn(__fmul_rn(b[2], fth), y0), fH);
                    b[3] = __fdiv_rn(__fadd_rn(__fmul_rn(b[3], ftw), x0), fW);
                }
                s_box[pos] = b;
                s_score[pos] = (unsigned)rec[4ll * T + row];
            }
            n += __popcll(votes);
        }
    }
    n = n < TM_CAP ? n : TM_CAP;
    __syncthreads();

    // ---- greedy NMS as rounds of arg-max: candidate lane + 64 j is bit j of this lane's mask
    const int nj = (n + 63) >> 6;
    unsigned live = 0;
    for (int j = 0; j < nj; ++j) live |= (lane + 64 * j < n) ? 1u << j : 0u;
    int *orec = p.out + (long long)f * words;
    const int slot0 = c * p.m;
    int k = 0;
    for (; k < p.m; ++k) {
        unsigned long long best = 0;            // (score order, ~index): no live candidate has key 0
        for (int j = 0; j < nj; ++j) {
            const int i = lane + 64 * j;
            if ((live >> j) & 1u) {
                const unsigned long long key = ((unsigned long long)score_order(s_score[i]) << 32) | (0xffffffffu - (unsigned)i);
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        if (best == 0) break;                   // wave-uniform
        const int w = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
        const v4f kept = s_box[w];
        if ((w & 63) == lane) live &= ~(1u << (w >> 6));
        const int slot = slot0 + k;
        if (lane < 4) orec[4ll * slot + lane] = __float_as_int(kept[lane]);
        if (lane == 4) orec[4ll * T + slot] = (int)s_score[w];
        if (lane == 5) orec[5ll * T + slot] = c;
        for (int j = 0; j < nj; ++j)
            if (((live >> j) & 1u) && iou_greater(s_box[lane + 64 * j], kept, p.thr)) live &= ~(1u << j);
    }
    // ---- the rows of this class that stay empty: zero, label -1 (tile_pack's mark)
    for (int e = k + lane; e < p.m; e += 64) {
        const int slot = slot0 + e;
#pragma unroll
        for (int q = 0; q < 4; ++q) orec[4ll * slot + q] = 0;
        orec[4ll * T + slot] = 0;
        orec[5ll * T + slot] = -1;
    }
}

__global__ __launch_bounds__(256) void tile_pack(int *__restrict__ out, int T)
{
    __shared__ int s_wave[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *rec = out + (long long)blockIdx.x * (6ll * T + 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    int count = 0;
    for (int start = 0; start < T; start += 256) {
        const int j = start + tid;
        const bool v = j < T && rec[5ll * T + j] >= 0;
        int b[4] = {0, 0, 0, 0}, sc = 0, lb = 0;
        if (v) {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = rec[4ll * j + q];
            sc = rec[4ll * T + j];
            lb = rec[5ll * T + j];
        }
        const unsigned long long votes = __ballot(v);
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();                        // every row of the chunk is in registers; the wave totals are visible
        int dest = count + __popcll(votes & below), total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            dest += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (v) {                                // dest <= j: a row this chunk or an earlier one has already read
#pragma unroll
            for (int q = 0; q < 4; ++q) rec[4ll * dest + q] = b[q];
            rec[4ll * T + dest] = sc;
            rec[5ll * T + dest] = lb;
        }
        count += total;
        __syncthreads();                        // s_wave is rewritten by the next chunk
    }
    for (int j = count + tid; j < T; j += 256) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rec[4ll * j + q] = 0;
        rec[4ll * T + j] = 0;
        rec[5ll * T + j] = 0;
    }
    if (tid == 0) rec[6ll * T] = count;
}

// the grid of include/ssd_hip.h and its refusals; `tiles`: F * ny * nx
int tile_grid(const std::string &who, int32_t F, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy, int32_t ox, TileGrid *g,
              int64_t *tiles)
{
    if (F < 1) return ssd_fail(SSD_ERR_INVALID, who + ": F must be at least 1");
    if (th < 128 || th % 128) return ssd_fail(SSD_ERR_INVALID, who + ": th must be a positive multiple of 128");
    if (tw < 128 || tw % 128) return ssd_fail(SSD_ERR_INVALID, who + ": tw must be a positive multiple of 128");
    if (H < th) return ssd_fail(SSD_ERR_INVALID, who + ": H is below th (a frame smaller than a tile is ssd_forward's)");
    if (W < tw) return ssd_fail(SSD_ERR_INVALID, who + ": W is below tw (a frame smaller than a tile is ssd_forward's)");
    if (oy < 0) return ssd_fail(SSD_ERR_INVALID, who + ": oy must not be negative");
    if (ox < 0) return ssd_fail(SSD_ERR_INVALID, who + ": ox must not be negative");
    if (th - oy < 1) return ssd_fail(SSD_ERR_INVALID, who + ": oy leaves a step th - oy below 1");
    if (tw - ox < 1) return ssd_fail(SSD_ERR_INVALID, who + ": ox leaves a step tw - ox below 1");
    if ((int64_t)F * H * W * 3 >= ((int64_t)1 << 31))
        return ssd_fail(SSD_ERR_INVALID, who + ": F * H * W * 3 must be below 2^31 bytes (the frame block is addressed with 32-bit offsets)");
    g->sy = th - oy;
    g->sx = tw - ox;
    g->ny = 1 + (H - th + g->sy - 1) / g->sy;
    g->nx = 1 + (W - tw + g->sx - 1) / g->sx;
    *tiles = (int64_t)F * g->ny * g->nx;
    if (*tiles > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": F * ny * nx must be below 2^31 tiles");
    return SSD_OK;
}

}  // namespace

extern "C" int ssd_tile_grid(int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy, int32_t ox, int32_t *grid_out)
{
    const std::string who = "ssd_tile_grid";
    if (!grid_out) return ssd_fail(SSD_ERR_INVALID, who + ": grid_out is NULL");
    TileGrid g;
    int64_t tiles;
    SSDCHK(tile_grid(who, 1, H, W, th, tw, oy, ox, &g, &tiles));
    grid_out[0] = g.ny;
    grid_out[1] = g.nx;
    grid_out[2] = g.sy;
    grid_out[3] = g.sx;
    return SSD_OK;
}

extern "C" int ssd_tile_gather(const uint8_t *frames_dev, int32_t F, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy, int32_t ox,
                               uint8_t *tiles_dev, void *stream)
{
    const std::string who = "ssd_tile_gather";
    if (!frames_dev) return ssd_fail(SSD_ERR_INVALID, who + ": frames_dev is NULL");
    if (!tiles_dev) return ssd_fail(SSD_ERR_INVALID, who + ": tiles_dev is NULL");
    if ((uintptr_t)tiles_dev & 3) return ssd_fail(SSD_ERR_INVALID, who + ": tiles_dev must be 4-byte aligned");
    TileGrid g;
    int64_t tiles;
    SSDCHK(tile_grid(who, F, H, W, th, tw, oy, ox, &g, &tiles));
    const int row_groups = tw * 3 / 16;                      // 3 * tw is a multiple of 384
    const long long groups = (long long)tiles * th * row_groups;
    const long long blocks = (groups + TG_THREADS - 1) / TG_THREADS;
    const unsigned grid = (unsigned)(blocks < TG_GRID_CAP ? blocks : TG_GRID_CAP);
    hipLaunchKernelGGL(tile_gather, dim3(grid), dim3(TG_THREADS), 0, (hipStream_t)stream, frames_dev, (int)((int64_t)F * H * W * 3), (int)H,
                       (int)W, (int)th, (int)tw, g, groups, row_groups, tiles_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}

extern "C" int ssd_tile_merge(const int32_t *tile_records_dev, const int32_t *full_records_dev, int32_t F, int32_t H, int32_t W, int32_t th,
                              int32_t tw, int32_t oy, int32_t ox, int32_t C, int32_t m, float iou_threshold, int32_t *out_records_dev,
                              void *stream)
{
    const std::string who = "ssd_tile_merge";
    if (!tile_records_dev) return ssd_fail(SSD_ERR_INVALID, who + ": tile_records_dev is NULL");
    if (!out_records_dev) return ssd_fail(SSD_ERR_INVALID, who + ": out_records_dev is NULL");
    if ((uintptr_t)tile_records_dev & 3) return ssd_fail(SSD_ERR_INVALID, who + ": tile_records_dev must be 4-byte aligned");
    if ((uintptr_t)full_records_dev & 3) return ssd_fail(SSD_ERR_INVALID, who + ": full_records_dev must be 4-byte aligned");
    if ((uintptr_t)out_records_dev & 3) return ssd_fail(SSD_ERR_INVALID, who + ": out_records_dev must be 4-byte aligned");
    if (C < 1) return ssd_fail(SSD_ERR_INVALID, who + ": C must be at least 1");
    if (m < 1) return ssd_fail(SSD_ERR_INVALID, who + ": m must be at least 1");
    if (iou_threshold != iou_threshold) return ssd_fail(SSD_ERR_INVALID, who + ": iou_threshold is NaN");
    TileGrid g;
    int64_t tiles;
    SSDCHK(tile_grid(who, F, H, W, th, tw, oy, ox, &g, &tiles));
    if (((int64_t)g.ny * g.nx + 1) * m > SSD_TILE_MAX_CANDIDATES)
        return ssd_fail(SSD_ERR_INVALID, who + ": (ny * nx + 1) * m = " + std::to_string(((int64_t)g.ny * g.nx + 1) * m) +
                                             " candidates of one class exceed SSD_TILE_MAX_CANDIDATES (" +
                                             std::to_string(SSD_TILE_MAX_CANDIDATES) + ")");
    if ((int64_t)C * m > (1 << 24)) return ssd_fail(SSD_ERR_INVALID, who + ": C * m must be at most 2^24");
    if ((int64_t)F * C > INT32_MAX) return ssd_fail(SSD_ERR_INVALID, who + ": F * C must be below 2^31");
    MergeArgs p;
    p.tiles = tile_records_dev;
    p.full = full_records_dev;
    p.out = out_records_dev;
    p.H = H; p.W = W; p.th = th; p.tw = tw;
    p.g = g;
    p.C = C; p.m = m; p.T = C * m;
    p.thr = iou_threshold;
    hipLaunchKernelGGL(tile_select, dim3((unsigned)(F * C)), dim3(64), 0, (hipStream_t)stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(tile_pack, dim3((unsigned)F), dim3(256), 0, (hipStream_t)stream, out_records_dev, p.T);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
