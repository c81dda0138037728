// The JPEG encoder's device stage: uint8 RGB frames -> quantised coefficients in the decoder's layout, two launches per batch
// whatever its size.  The arithmetic of every stage, the dummy-block rule, the table and every refusal: include/ssd_hip.h, block
// "the JPEG encoder".
//
//   jpeg_enc_planes  a 256-lane group takes one tile of SSD_JPEG_ENC_TILE units of ONE image (the table's tile_begin, a wave-uniform
//                    search), so the sampling -- 4:4:4 or 4:2:0 -- is a uniform branch to one instantiation of the unit.  A lane
//                    owns one unit: 8 consecutive chroma samples of one row of the padded chroma plane and the 8 h by v luma
//                    samples they cover.  It reads the pixels bytewise with the coordinates clamped to the frame (which IS the
//                    edge replication; for 4:2:0 the chroma ROW is clamped to the last real downsampled row first), and stores
//                    8 bytes per chroma plane and 8 h bytes per luma row.  Every sample of the padded planes is written.
//   jpeg_enc_fdct    256 lanes = 32 blocks of 8 lanes, as jpeg.hip's jpeg_idct: a grid of at most WAVE_GRID_CAP groups strides over
//                    ALL blocks of all components of all images (block_begin: one binary search per lane, then a forward walk).
//                    Lane r loads row r of the block (8 bytes), runs pass 1 on it in registers and writes the row into the
//                    block's LDS tile of pitch 9 words; lane c runs pass 2 on column c in place; lane r reads row r back,
//                    divides by row r of the base table scaled by the image's quality (jpeg_quant.h: the rule the host stage
//                    writes into DQT) and stores the 8 int16 as one 16-byte store.  A dummy block stores zeros
//                    and reads nothing.  Only the lanes of ONE wave share a tile: no __syncthreads.
// No atomics, every output byte written once: two calls give the same bytes.
#include "metric_host.h"
#include "jpeg_geom.h"
#include "jpeg_table.h"
#include "jpeg_quant.h"

namespace {

constexpr int ET = 256;
constexpr int E_BLOCKS = ET / 8;                // blocks of a group per pass
constexpr int E_PITCH = 9;                      // words between the rows of a block's LDS tile
static_assert(SSD_JPEG_ENC_TILE == ET, "a lane per unit");

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));

__constant__ __attribute__((aligned(16))) uint8_t c_base_q[2][64] = JPEG_BASE_Q_INIT;      // Annex K.1: luma, chroma; natural order

struct Ycc { unsigned y, cb, cr; };

__device__ __forceinline__ Ycc convert(const uint8_t *__restrict__ px)
{
    const unsigned r = px[0], g = px[1], b = px[2];
    Ycc o;
    o.y = (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
    o.cb = ((128u << 16) + 32767u + 32768u * b - 11059u * r - 21709u * g) >> 16;
    o.cr = ((128u << 16) + 32767u + 32768u * r - 27439u * g - 5329u * b) >> 16;
    return o;
}

// One unit of image `im`: chroma row cy, chroma columns [8 cx8, 8 cx8 + 8) of the padded plane.  HV 1: 4:4:4, 2: 4:2:0.
template <int HV>
__device__ __forceinline__ void plane_unit(const ssd_jpeg_encode_image &im, const uint8_t *__restrict__ frame, uint8_t *__restrict__ planes,
                                           int cy, int cx8)
{
    const int H = im.height, W = im.width;
    const int64_t mcus = (int64_t)im.mcus_x * im.mcus_y;
    const int pitch_c = im.mcus_x * 8, pitch_y = pitch_c * HV;
    uint8_t *py = planes, *pcb = planes + 64 * mcus * HV * HV, *pcr = pcb + 64 * mcus;
    unsigned cb[2] = {0, 0}, cr[2] = {0, 0};
    if (HV == 1) {
        const uint8_t *row = frame + 3 * (int64_t)min(cy, H - 1) * W;
        unsigned yy[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const Ycc s = convert(row + 3 * min(8 * cx8 + k, W - 1));
            yy[k >> 2] |= s.y << (8 * (k & 3));
            cb[k >> 2] |= s.cb << (8 * (k & 3));
            cr[k >> 2] |= s.cr << (8 * (k & 3));
        }
        uint2_t v;
        v.x = yy[0], v.y = yy[1];
        *reinterpret_cast<uint2_t *>(py + (int64_t)cy * pitch_y + 8 * cx8) = v;
    } else {
        // the chroma row: the last REAL downsampled row continues downwards; its two source rows clamp to the frame
        const int j = min(cy, ((H + 1) >> 1) - 1);
        const uint8_t *row0 = frame + 3 * (int64_t)min(2 * j, H - 1) * W, *row1 = frame + 3 * (int64_t)min(2 * j + 1, H - 1) * W;
        // the two luma rows this unit covers: full-size, clamped one by one
        const uint8_t *lrow0 = frame + 3 * (int64_t)min(2 * cy, H - 1) * W, *lrow1 = frame + 3 * (int64_t)min(2 * cy + 1, H - 1) * W;
        const bool same = lrow0 == row0 && lrow1 == row1;                    // all but the rows below an even height's last pair
        unsigned y0[4] = {0, 0, 0, 0}, y1[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int x0 = min(16 * cx8 + 2 * k, W - 1), x1 = min(16 * cx8 + 2 * k + 1, W - 1);
            const Ycc a = convert(row0 + 3 * x0), b = convert(row0 + 3 * x1), c = convert(row1 + 3 * x0), d = convert(row1 + 3 * x1);
            const unsigned bias = 1u + (k & 1);
            cb[k >> 2] |= ((a.cb + b.cb + c.cb + d.cb + bias) >> 2) << (8 * (k & 3));
            cr[k >> 2] |= ((a.cr + b.cr + c.cr + d.cr + bias) >> 2) << (8 * (k & 3));
            unsigned l00 = a.y, l01 = b.y, l10 = c.y, l11 = d.y;
            if (!same) {
                l00 = convert(lrow0 + 3 * x0).y, l01 = convert(lrow0 + 3 * x1).y;
                l10 = convert(lrow1 + 3 * x0).y, l11 = convert(lrow1 + 3 * x1).y;
            }
            y0[k >> 1] |= (l00 | (l01 << 8)) << (16 * (k & 1));
            y1[k >> 1] |= (l10 | (l11 << 8)) << (16 * (k & 1));
        }
        uint4_t v0, v1;
        v0.x = y0[0], v0.y = y0[1], v0.z = y0[2], v0.w = y0[3];
        v1.x = y1[0], v1.y = y1[1], v1.z = y1[2], v1.w = y1[3];
        *reinterpret_cast<uint4_t *>(py + (int64_t)(2 * cy) * pitch_y + 16 * cx8) = v0;
        *reinterpret_cast<uint4_t *>(py + (int64_t)(2 * cy + 1) * pitch_y + 16 * cx8) = v1;
    }
    uint2_t vb, vr;
    vb.x = cb[0], vb.y = cb[1];
    vr.x = cr[0], vr.y = cr[1];
    *reinterpret_cast<uint2_t *>(pcb + (int64_t)cy * pitch_c + 8 * cx8) = vb;
    *reinterpret_cast<uint2_t *>(pcr + (int64_t)cy * pitch_c + 8 * cx8) = vr;
}

__global__ __launch_bounds__(ET) void jpeg_enc_planes(const ssd_jpeg_encode_image *__restrict__ images, int B, int64_t total,
                                                      const uint8_t *__restrict__ frames, uint8_t *__restrict__ ws)
{
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int i = find_row(B, t, [&](int k) { return images[k].tile_begin; });          // wave-uniform
        const ssd_jpeg_encode_image im = images[i];
        const int64_t u = (t - im.tile_begin) * ET + threadIdx.x;
        if (u >= 8 * (int64_t)im.mcus_y * im.mcus_x) continue;
        const int cy = (int)(u / im.mcus_x), cx8 = (int)(u % im.mcus_x);
        if (im.h == 1) plane_unit<1>(im, frames + im.frame_offset, ws + im.plane_offset, cy, cx8);
        else plane_unit<2>(im, frames + im.frame_offset, ws + im.plane_offset, cy, cx8);
    }
}

// the one-dimensional kernel of the header, in uint32 (nothing relies on signed overflow); FIRST: pass 1's scaling
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int *d, int *o)
{
    constexpr int N = FIRST ? 11 : 15;
    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], d5 = d[5], d6 = d[6], d7 = d[7];
    const uint32_t t0 = d0 + d7, t1 = d1 + d6, t2 = d2 + d5, t3 = d3 + d4;
    uint32_t t7 = d0 - d7, t6 = d1 - d6, t5 = d2 - d5, t4 = d3 - d4;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const auto descale = [](uint32_t x, int n) { return (int)(x + (1u << (n - 1))) >> n; };
    o[0] = FIRST ? (int)((t10 + t11) << 2) : descale(t10 + t11, 2);
    o[4] = FIRST ? (int)((t10 - t11) << 2) : descale(t10 - t11, 2);
    uint32_t z1 = (t12 + t13) * 4433u;
    o[2] = descale(z1 + t13 * 6270u, N);
    o[6] = descale(z1 - t12 * 15137u, N);
    z1 = t4 + t7;
    uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const uint32_t z5 = (z3 + z4) * 9633u;
    t4 *= 2446u, t5 *= 16819u, t6 *= 25172u, t7 *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
    o[7] = descale(t4 + z1 + z3, N);
    o[5] = descale(t5 + z2 + z4, N);
    o[3] = descale(t6 + z2 + z3, N);
    o[1] = descale(t7 + z1 + z4, N);
}

__global__ __launch_bounds__(ET) void jpeg_enc_fdct(const ssd_jpeg_encode_image *__restrict__ images, int B, int64_t total,
                                                    const uint8_t *__restrict__ ws, int16_t *__restrict__ coef)
{
    __shared__ int s_tile[E_BLOCKS * 8 * E_PITCH];
    const int slot = (int)threadIdx.x >> 3, r = (int)threadIdx.x & 7;
    int *tile = s_tile + slot * 8 * E_PITCH;
    const int64_t stride = (int64_t)gridDim.x * E_BLOCKS;
    int i = -1;
    int64_t next_begin = 0;
    for (int64_t g0 = (int64_t)blockIdx.x * E_BLOCKS; g0 < total; g0 += stride) {
        const int64_t g = g0 + slot;
        const bool active = g < total;
        bool real = false;
        int x[8] = {0, 0, 0, 0, 0, 0, 0, 0}, chroma = 0, scale = 100;
        int16_t *dst = nullptr;
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
            const ssd_jpeg_encode_image im = images[i];
            const int64_t local = g - im.block_begin;
            const int64_t mcus = (int64_t)im.mcus_x * im.mcus_y;
            const int64_t n0 = mcus * im.h * im.v;
            const int comp = local < n0 ? 0 : local < n0 + mcus ? 1 : 2;
            const int64_t before = comp == 0 ? 0 : comp == 1 ? n0 : n0 + mcus;
            const int64_t lb = local - before;
            const int row_blocks = comp == 0 ? im.mcus_x * im.h : im.mcus_x;
            const int by = (int)(lb / row_blocks), bx = (int)(lb % row_blocks);
            // the component's own whole blocks; the rest of its padded grid are dummy blocks (luma of 4:2:0 only)
            real = comp != 0 || (bx < (im.width + 7) / 8 && by < (im.height + 7) / 8);
            chroma = comp != 0;
            scale = jpeg_quality_scale(im.quality);
            dst = coef + im.coef_offset + local * 64 + r * 8;
            if (real) {
                const uint2_t sv = *reinterpret_cast<const uint2_t *>(ws + im.plane_offset + 64 * before +
                                                                      ((int64_t)by * 8 + r) * ((int64_t)row_blocks * 8) + (int64_t)bx * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[k] = (int)((sv.x >> (8 * k)) & 255u) - 128;
                    x[k + 4] = (int)((sv.y >> (8 * k)) & 255u) - 128;
                }
            }
        }
        // pass 1: this lane's row, from its registers
        int o[8];
        fdct_1d<true>(x, o);
#pragma unroll
        for (int c = 0; c < 8; ++c) tile[r * E_PITCH + c] = o[c];
        wave_lds_sync();
        // pass 2: this lane's column, in place
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = tile[k * E_PITCH + r];
        fdct_1d<false>(x, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * E_PITCH + r] = o[k];
        wave_lds_sync();
        // this lane's row again: / (8 q), halves away from zero
        const uint2_t bv = *reinterpret_cast<const uint2_t *>(&c_base_q[chroma][8 * r]);
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int val = tile[r * E_PITCH + c];
            const unsigned d = 8u * (unsigned)jpeg_quant_entry((int)((bv[c >> 2] >> (8 * (c & 3))) & 0xffu), scale);
            const unsigned mag = ((unsigned)(val < 0 ? -val : val) + (d >> 1)) / d;
            const unsigned q16 = (val < 0 ? 0u - mag : mag) & 0xffffu;
            w[c >> 1] |= q16 << (16 * (c & 1));
        }
        if (active) {
            uint4_t v;
            v.x = real ? w[0] : 0u, v.y = real ? w[1] : 0u, v.z = real ? w[2] : 0u, v.w = real ? w[3] : 0u;
            *reinterpret_cast<uint4_t *>(dst) = v;
        }
        // (the next pass writes row r of the tile from this lane only, behind its own reads above: no third sync)
    }
}

int64_t image_blocks(const ssd_jpeg_encode_image &f)
{
    return jpeg_luma_blocks(f.h, f.v, f.mcus_x, f.mcus_y) + 2 * jpeg_chroma_blocks(3, f.mcus_x, f.mcus_y);
}

// SSD_OK and the batch's totals, or the reason
int check_table(const std::string &who, const ssd_jpeg_encode_image *im, int32_t B, int64_t *blocks_out, int64_t *tiles_out, int64_t *ws_out)
{
    if (B < 0 || B > (1 << 20)) return ssd_fail(SSD_ERR_INVALID, who + ": B must be in [0, 2^20]");
    if (B > 0 && !im) return ssd_fail(SSD_ERR_INVALID, who + ": images_host is NULL");
    int64_t blocks = 0, tiles = 0, plane_end = 0, coef_end = 0;
    for (int32_t b = 0; b < B; ++b) {
        const ssd_jpeg_encode_image &f = im[b];
        const std::string row = who + ": images_host[" + std::to_string(b) + "]";
        if (!((f.h == 1 && f.v == 1) || (f.h == 2 && f.v == 2)))
            return ssd_fail(SSD_ERR_UNSUPPORTED, row + ": the sampling must be 4:4:4 (1x1) or 4:2:0 (2x2)");
        if (!jpeg_geometry_ok(f.height, f.width, 3, f.h, f.v, f.mcus_x, f.mcus_y))
            return ssd_fail(SSD_ERR_INVALID, row + ": height and width must be in [1, 65535], mcus_x and mcus_y their MCU counts");
        if (f.quality < 1 || f.quality > 100) return ssd_fail(SSD_ERR_INVALID, row + ".quality must be in [1, 100]");
        const int64_t nb = image_blocks(f), units = 8 * (int64_t)f.mcus_y * f.mcus_x;
        if (f.frame_offset < 0 || f.frame_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".frame_offset must be in [0, 2^40]");
        if (f.plane_offset < plane_end || (f.plane_offset & 15) || f.plane_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".plane_offset must be a multiple of 16 behind the planes before it");
        if (f.coef_offset < coef_end || (f.coef_offset & 7) || f.coef_offset > ((int64_t)1 << 40))
            return ssd_fail(SSD_ERR_INVALID, row + ".coef_offset must be a multiple of 8 behind the coefficients before it");
        if (f.block_begin != blocks) return ssd_fail(SSD_ERR_INVALID, row + ".block_begin must be the blocks of the images before");
        if (f.tile_begin != tiles) return ssd_fail(SSD_ERR_INVALID, row + ".tile_begin must be the tiles of the images before");
        blocks += nb;
        tiles += (units + SSD_JPEG_ENC_TILE - 1) / SSD_JPEG_ENC_TILE;
        plane_end = f.plane_offset + 64 * nb;
        coef_end = f.coef_offset + 64 * nb;
    }
    *blocks_out = blocks, *tiles_out = tiles, *ws_out = plane_end;
    return SSD_OK;
}

}  // namespace

extern "C" size_t ssd_jpeg_encode_workspace_bytes(const ssd_jpeg_encode_image *images_host, int32_t B)
{
    int64_t blocks, tiles, ws;
    if (check_table("ssd_jpeg_encode_workspace_bytes", images_host, B, &blocks, &tiles, &ws) != SSD_OK) return 0;
    return (size_t)ws;
}

extern "C" int ssd_jpeg_encode(const ssd_jpeg_encode_image *images_host, const ssd_jpeg_encode_image *images_dev, int32_t B,
                               const uint8_t *frames_dev, void *workspace_dev, int16_t *coef_dev, void *stream)
{
    const std::string who = "ssd_jpeg_encode";
    int64_t blocks, tiles, ws;
    SSDCHK(check_table(who, images_host, B, &blocks, &tiles, &ws));
    SSDCHK(check_ptrs(who, {{images_dev, B > 0, 8, "images_dev"}, {frames_dev, B > 0, 1, "frames_dev"},
                            {workspace_dev, B > 0, 16, "workspace_dev"}, {coef_dev, B > 0, 16, "coef_dev"}}));
    if (B == 0) return SSD_OK;
    hipLaunchKernelGGL(jpeg_enc_planes, dim3(capped_grid(tiles)), dim3(ET), 0, (hipStream_t)stream, images_dev, (int)B, tiles, frames_dev,
                       (uint8_t *)workspace_dev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_fdct, dim3(capped_grid((blocks + E_BLOCKS - 1) / E_BLOCKS)), dim3(ET), 0, (hipStream_t)stream, images_dev,
                       (int)B, blocks, (const uint8_t *)workspace_dev, coef_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
