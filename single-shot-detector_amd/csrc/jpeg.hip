// The JPEG decoder's device stage: quantised coefficients -> uint8 RGB frames, two launches per batch whatever its size.
// The arithmetic (IDCT, upsampling, colour), the table and every refusal: include/ssd_hip.h, block "the JPEG decoder".
//
//   jpeg_idct     256 lanes = 32 blocks of 8 lanes; a grid of at most WAVE_GRID_CAP groups (metric_host.h) strides over ALL blocks of all
//                 components of all images (the table's block_begin: one binary search per lane, then a forward walk).
//                 Lane r of a block loads row r of the coefficients and of the component's table (16 bytes each: a wave reads 8
//                 blocks as 1 KiB in a row), multiplies, and writes the row into the block's LDS tile of pitch 9 words -- the
//                 eight lanes of a block and the eight blocks of a wave then hit 64 different banks on the row writes, the
//                 column reads and the row reads alike.  Lane c runs pass 1 on column c in place, lane r pass 2 on row r, and
//                 stores the row's 8 samples as one 8-byte store into the component's plane (pitch 8 * blocks per row).
//                 Only the lanes of ONE wave share a tile: no __syncthreads.
//   jpeg_pixels   a 256-lane group takes one tile of SSD_JPEG_TILE consecutive pixels of ONE frame (the table's tile_begin, a
//                 wave-uniform search), so the image's mode -- gray, 4:4:4, 4:2:2, 4:2:0, replicate -- is a uniform branch to
//                 one instantiation of the pixel loop.  A lane owns SSD_JPEG_RUN consecutive pixels in row-major order: 48
//                 bytes at a multiple of 48 from the frame's 16-byte aligned base, three 16-byte stores; the last, shorter run
//                 of a frame stores its bytes singly, so no byte outside a frame is written.  Chroma neighbours are clamped to
//                 the real extent, which IS the edge rule of the header (3 c + c = 4 c).
// No atomics, every output byte written once: two calls give the same bytes.
#include "metric_host.h"
#include "jpeg_geom.h"
#include "jpeg_table.h"

namespace {

constexpr int JT = 256;
constexpr int J_BLOCKS = JT / 8;                // blocks of a group per pass
constexpr int J_PITCH = 9;                      // words between the rows of a block's LDS tile
static_assert(SSD_JPEG_TILE == JT * SSD_JPEG_RUN, "a lane per run");

// the one-dimensional kernel of the header, in uint32 (the sums wrap, nothing relies on signed overflow)
__device__ __forceinline__ void idct_1d(const int *x, uint32_t *o)
{
    const uint32_t x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4], x5 = x[5], x6 = x[6], x7 = x[7];
    uint32_t z1 = (x2 + x6) * 4433u;
    const uint32_t t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
    const uint32_t t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = x7, b = x5, c = x3, d = x1;
    z1 = a + d;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a *= 2446u, b *= 16819u, c *= 25172u, d *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
    a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
    o[0] = t10 + d, o[1] = t11 + c, o[2] = t12 + b, o[3] = t13 + a;
    o[4] = t13 - a, o[5] = t12 - b, o[6] = t11 - c, o[7] = t10 - d;
}

typedef int int4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ __launch_bounds__(JT) void jpeg_idct(const ssd_jpeg_image *__restrict__ images, int B, int64_t total,
                                                const int16_t *__restrict__ coef, const uint16_t *__restrict__ quant,
                                                uint8_t *__restrict__ ws)
{
    __shared__ int s_tile[J_BLOCKS * 8 * J_PITCH];
    const int slot = (int)threadIdx.x >> 3, r = (int)threadIdx.x & 7;
    int *tile = s_tile + slot * 8 * J_PITCH;
    const int64_t stride = (int64_t)gridDim.x * J_BLOCKS;
    int i = -1;
    int64_t next_begin = 0;
    for (int64_t g0 = (int64_t)blockIdx.x * J_BLOCKS; g0 < total; g0 += stride) {
        const int64_t g = g0 + slot;
        const bool active = g < total;
        int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint8_t *dst = nullptr;
        if (active) {
            // image i holds blocks [block_begin(i), next_begin); every image has blocks and g < total, so the walk ends at i <= B - 1
            if (i < 0) {
                i = find_row(B, g, [&](int k) { return images[k].block_begin; });
                next_begin = i + 1 < B ? images[i + 1].block_begin : total;
            }
            while (g >= next_begin) {
                ++i;
                next_begin = i + 1 < B ? images[i + 1].block_begin : total;
            }
            const ssd_jpeg_image im = images[i];
            const int64_t local = g - im.block_begin;
            const int64_t mcus = (int64_t)im.mcus_x * im.mcus_y;
            const int64_t n0 = mcus * im.h * im.v, n1 = im.components == 3 ? mcus : 0;
            const int comp = local < n0 ? 0 : local < n0 + n1 ? 1 : 2;
            const int64_t before = comp == 0 ? 0 : comp == 1 ? n0 : n0 + n1;
            const int64_t lb = local - before;
            const int row_blocks = comp == 0 ? im.mcus_x * im.h : im.mcus_x;
            const int by = (int)(lb / row_blocks), bx = (int)(lb % row_blocks);
            const int4_t cv = *reinterpret_cast<const int4_t *>(coef + im.coef_offset + local * 64 + r * 8);
            const uint4_t qv = *reinterpret_cast<const uint4_t *>(quant + im.quant_offset + comp * 64 + r * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c2 = cv[k];
                const unsigned q2 = qv[k];
                x[2 * k] = (int)(short)(c2 & 0xffff) * (int)(q2 & 0xffffu);
                x[2 * k + 1] = (c2 >> 16) * (int)(q2 >> 16);
            }
            dst = ws + im.plane_offset + 64 * before + ((int64_t)by * 8 + r) * ((int64_t)row_blocks * 8) + (int64_t)bx * 8;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) tile[r * J_PITCH + c] = x[c];
        wave_lds_sync();
        // pass 1: this lane's column, in place
        uint32_t o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = tile[k * J_PITCH + r];
        idct_1d(x, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * J_PITCH + r] = (int)(o[k] + (1u << 10)) >> 11;
        wave_lds_sync();
        // pass 2: this lane's row
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = tile[r * J_PITCH + c];
        idct_1d(x, o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (unsigned)clamp255(((int)(o[c] + (1u << 17)) >> 18) + 128) << (8 * c);
            hi |= (unsigned)clamp255(((int)(o[c + 4] + (1u << 17)) >> 18) + 128) << (8 * c);
        }
        if (active) {
            uint2_t v;
            v.x = lo, v.y = hi;
            *reinterpret_cast<uint2_t *>(dst) = v;
        }
        // (the next pass writes row r of the tile from this lane only, behind its own reads above: no third sync)
    }
}

struct Planes {
    const uint8_t *y, *cb, *cr;
    int pitch_y, pitch_c;
    int H, W, n, m;             // n, m: the chroma planes' real extents
};

// MODE 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0, 4 / 5: 4:2:2 / 4:2:0 at n <= 2 (each sample replicated)
template <int MODE>
__device__ __forceinline__ void chroma_at(const Planes &p, int y, int x, int &cb, int &cr)
{
    if (MODE == 1) {
        cb = p.cb[(int64_t)y * p.pitch_c + x];
        cr = p.cr[(int64_t)y * p.pitch_c + x];
    } else if (MODE == 4 || MODE == 5) {
        const int64_t at = (int64_t)(MODE == 5 ? y >> 1 : y) * p.pitch_c + (x >> 1);
        cb = p.cb[at];
        cr = p.cr[at];
    } else if (MODE == 2) {
        const int i = x >> 1, odd = x & 1;
        const int ii = odd ? min(i + 1, p.n - 1) : max(i - 1, 0);
        const int64_t row = (int64_t)y * p.pitch_c;
        cb = (3 * p.cb[row + i] + p.cb[row + ii] + 1 + odd) >> 2;
        cr = (3 * p.cr[row + i] + p.cr[row + ii] + 1 + odd) >> 2;
    } else if (MODE == 3) {
        const int j = y >> 1, i = x >> 1, odd = x & 1;
        const int nb = (y & 1) ? min(j + 1, p.m - 1) : max(j - 1, 0);
        const int ii = odd ? min(i + 1, p.n - 1) : max(i - 1, 0);
        const int64_t r0 = (int64_t)j * p.pitch_c, r1 = (int64_t)nb * p.pitch_c;
        const int b0 = 3 * p.cb[r0 + i] + p.cb[r1 + i], b1 = 3 * p.cb[r0 + ii] + p.cb[r1 + ii];
        const int c0 = 3 * p.cr[r0 + i] + p.cr[r1 + i], c1 = 3 * p.cr[r0 + ii] + p.cr[r1 + ii];
        cb = (3 * b0 + b1 + 8 - odd) >> 4;
        cr = (3 * c0 + c1 + 8 - odd) >> 4;
    }
}

template <int MODE>
__device__ __forceinline__ void pixel_run(const Planes &p, int64_t p0, int count, uint8_t *__restrict__ frame)
{
    int y = (int)(p0 / p.W), x = (int)(p0 % p.W);
    unsigned w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // the run's 48 bytes
#pragma unroll
    for (int k = 0; k < SSD_JPEG_RUN; ++k) {
        if (k < count) {
            const int Y = p.y[(int64_t)y * p.pitch_y + x];
            int R = Y, G = Y, Bl = Y;
            if (MODE != 0) {
                int cb = 0, cr = 0;
                chroma_at<MODE>(p, y, x, cb, cr);
                cb -= 128, cr -= 128;
                R = clamp255(Y + ((91881 * cr + 32768) >> 16));
                G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                Bl = clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
            w[(3 * k) >> 2] |= (unsigned)R << (8 * ((3 * k) & 3));
            w[(3 * k + 1) >> 2] |= (unsigned)G << (8 * ((3 * k + 1) & 3));
            w[(3 * k + 2) >> 2] |= (unsigned)Bl << (8 * ((3 * k + 2) & 3));
            if (++x == p.W) x = 0, ++y;
        }
    }
    uint8_t *out = frame + 3 * p0;
    if (count == SSD_JPEG_RUN) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint4_t v;
            v.x = w[4 * k], v.y = w[4 * k + 1], v.z = w[4 * k + 2], v.w = w[4 * k + 3];
            reinterpret_cast<uint4_t *>(out)[k] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * SSD_JPEG_RUN; ++k)
            if (k < 3 * count) out[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

__global__ __launch_bounds__(JT) void jpeg_pixels(const ssd_jpeg_image *__restrict__ images, int B, int64_t total,
                                                  const uint8_t *__restrict__ ws, uint8_t *__restrict__ frames)
{
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int i = find_row(B, t, [&](int k) { return images[k].tile_begin; });          // wave-uniform
        const ssd_jpeg_image im = images[i];
        const int64_t npx = (int64_t)im.height * im.width;
        const int64_t p0 = ((t - im.tile_begin) * JT + threadIdx.x) * SSD_JPEG_RUN;
        if (p0 >= npx) continue;
        const int count = (int)(npx - p0 < SSD_JPEG_RUN ? npx - p0 : SSD_JPEG_RUN);
        const int64_t mcus = (int64_t)im.mcus_x * im.mcus_y;
        Planes p;
        p.y = ws + im.plane_offset;
        p.cb = p.y + 64 * mcus * im.h * im.v;
        p.cr = p.cb + 64 * mcus;
        p.pitch_y = im.mcus_x * im.h * 8;
        p.pitch_c = im.mcus_x * 8;
        p.H = im.height, p.W = im.width;
        p.n = (im.width + 1) >> 1, p.m = (im.height + 1) >> 1;
        uint8_t *frame = frames + im.frame_offset;
        const int mode = im.components == 1 ? 0 : im.h == 1 ? 1 : (im.v == 1 ? 2 : 3) + (p.n <= 2 ? 2 : 0);
        switch (mode) {
        case 0: pixel_run<0>(p, p0, count, frame); break;
        case 1: pixel_run<1>(p, p0, count, frame); break;
        case 2: pixel_run<2>(p, p0, count, frame); break;
        case 3: pixel_run<3>(p, p0, count, frame); break;
        case 4: pixel_run<4>(p, p0, count, frame); break;
        default: pixel_run<5>(p, p0, count, frame); break;
        }
    }
}

bool geometry_ok(const ssd_jpeg_image &f) { return jpeg_geometry_ok(f.height, f.width, f.components, f.h, f.v, f.mcus_x, f.mcus_y); }

int64_t image_blocks(const ssd_jpeg_image &f)
{
    return jpeg_luma_blocks(f.h, f.v, f.mcus_x, f.mcus_y) + 2 * jpeg_chroma_blocks(f.components, f.mcus_x, f.mcus_y);
}

// SSD_OK and the batch's totals, or the reason
int check_table(const std::string &who, const ssd_jpeg_image *im, int32_t B, int64_t *blocks_out, int64_t *tiles_out, int64_t *ws_out)
{
    if (B < 0 || B > (1 << 20)) return ssd_fail(SSD_ERR_INVALID, who + ": B must be in [0, 2^20]");
    if (B > 0 && !im) return ssd_fail(SSD_ERR_INVALID, who + ": images_host is NULL");
    int64_t blocks = 0, tiles = 0, plane_end = 0, frame_end = 0;
    for (int32_t b = 0; b < B; ++b) {
        const ssd_jpeg_image &f = im[b];
        const std::string row = who + ": images_host[" + std::to_string(b) + "]";
        if (!geometry_ok(f)) return ssd_fail(SSD_ERR_INVALID, row + ": a geometry no accepted stream gives");
        const int64_t nb = image_blocks(f), px = (int64_t)f.height * f.width;
        if (f.coef_offset < 0 || (f.coef_offset & 7) || f.coef_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".coef_offset must be a multiple of 8 in [0, 2^40]");
        if (f.quant_offset < 0 || (f.quant_offset & 7) || f.quant_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".quant_offset must be a multiple of 8 in [0, 2^40]");
        if (f.plane_offset < plane_end || (f.plane_offset & 7) || f.plane_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".plane_offset must be a multiple of 8 behind the planes before it");
        if (f.frame_offset < frame_end || (f.frame_offset & 15) || f.frame_offset + 3 * px > 0x7fffffffLL)
            return ssd_fail(SSD_ERR_INVALID, row + ".frame_offset must be a multiple of 16 behind the frames before it, the frame ending below 2^31");
        if (f.block_begin != blocks) return ssd_fail(SSD_ERR_INVALID, row + ".block_begin must be the blocks of the images before");
        if (f.tile_begin != tiles) return ssd_fail(SSD_ERR_INVALID, row + ".tile_begin must be the tiles of the images before");
        blocks += nb;
        tiles += (px + SSD_JPEG_TILE - 1) / SSD_JPEG_TILE;
        plane_end = f.plane_offset + 64 * nb;
        frame_end = f.frame_offset + 3 * px;
    }
    *blocks_out = blocks, *tiles_out = tiles, *ws_out = (plane_end + 15) & ~(int64_t)15;
    return SSD_OK;
}

}  // namespace

extern "C" size_t ssd_jpeg_workspace_bytes(const ssd_jpeg_image *images_host, int32_t B)
{
    int64_t blocks, tiles, ws;
    if (check_table("ssd_jpeg_workspace_bytes", images_host, B, &blocks, &tiles, &ws) != SSD_OK) return 0;
    return (size_t)ws;
}

extern "C" int ssd_jpeg_decode(const ssd_jpeg_image *images_host, const ssd_jpeg_image *images_dev, int32_t B, const int16_t *coef_dev,
                               const uint16_t *quant_dev, void *workspace_dev, uint8_t *frames_dev, void *stream)
{
    const std::string who = "ssd_jpeg_decode";
    int64_t blocks, tiles, ws;
    SSDCHK(check_table(who, images_host, B, &blocks, &tiles, &ws));
    SSDCHK(check_ptrs(who, {{images_dev, B > 0, 8, "images_dev"}, {coef_dev, B > 0, 16, "coef_dev"}, {quant_dev, B > 0, 16, "quant_dev"},
                            {workspace_dev, B > 0, 16, "workspace_dev"}, {frames_dev, B > 0, 16, "frames_dev"}}));
    if (B == 0) return SSD_OK;
    hipLaunchKernelGGL(jpeg_idct, dim3(capped_grid((blocks + J_BLOCKS - 1) / J_BLOCKS)), dim3(JT), 0, (hipStream_t)stream,
                       images_dev, (int)B, blocks, coef_dev, quant_dev, (uint8_t *)workspace_dev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_pixels, dim3(capped_grid(tiles)), dim3(JT), 0,
                       (hipStream_t)stream, images_dev, (int)B, tiles, (const uint8_t *)workspace_dev, frames_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
