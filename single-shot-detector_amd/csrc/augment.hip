// The TRAIN input pipeline's per-pixel work (pipeline.py:117-135 after the decode): crop, nearest-neighbour resize, uint8 ->
// [0, 1], colour offsets, grayscale, per-element random scale, horizontal flip -- one launch per batch.  Semantics:
// include/ssd_hip.h, block "the TRAIN input pipeline".
//
//   augment   one lane per 4 consecutive output pixels of a row (a "quad"), 256 lanes per block, every block inside ONE image
//             (out_h * out_w is a multiple of 16 384, so an image is a whole number of blocks): the image's parameters and its
//             flags are block-uniform.  The 12 source bytes are gathered as single-byte buffer loads (frames start at any byte
//             offset: nothing depends on the device's unaligned-access mode); the quad's 12 floats leave as three 16-byte stores (NHWC: 48 contiguous bytes) or one
//             16-byte store per plane (NCHW).  A flipped quad is the mirrored quad with its pixels reversed, so it stays
//             aligned.  No LDS, no atomics; Philox runs only in blocks of images with the scale flag.
#include "host.h"

#pragma clang fp contract(off)

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PIXELS = 4 * AUG_THREADS;           // output pixels per block
constexpr int32_t AUG_FLAGS = SSD_AUG_COLOR | SSD_AUG_GRAY | SSD_AUG_SCALE | SSD_AUG_FLIP;
static_assert(sizeof(ssd_augment_params) == 64, "ssd_augment_params is the 64-byte row of include/ssd_hip.h");

// Philox4x32-10 (Salmon et al., SC'11) on the counter (c0, 0, 0, 0): 10 rounds, the key bumped between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t (&r)[4])
{
    uint32_t c[4] = {c0, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    r[0] = c[0]; r[1] = c[1]; r[2] = c[2]; r[3] = c[3];
}

// TF's Uint32ToFloat: 23 random mantissa bits under exponent 0 -> [1, 2), minus 1
__device__ __forceinline__ float uint_to_unit(uint32_t w) { return __uint_as_float(0x3f800000u | (w & 0x7fffffu)) - 1.0f; }

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// the project's nearest-neighbour index (first_pixels.h fc_src): min(floor(dst * (in / out)), in - 1)
__device__ __forceinline__ int nn_src(int dst, float scale, int n)
{
    const int v = (int)floorf((float)dst * scale);
    return v < n - 1 ? v : n - 1;
}

__global__ __launch_bounds__(AUG_THREADS) void augment(const uint8_t *__restrict__ images, const ssd_augment_params *__restrict__ params,
                                                       int out_h, int out_w, int blocks_per_image, int channels_first,
                                                       float *__restrict__ out)
{
    const int b = (int)blockIdx.x / blocks_per_image;
    const int q = ((int)blockIdx.x - b * blocks_per_image) * AUG_THREADS + (int)threadIdx.x;     // quad of image b
    const ssd_augment_params p = params[b];
    const int quads_per_row = out_w >> 2;
    const int y = q / quads_per_row, x = (q - y * quads_per_row) << 2;
    const float hs = __fdiv_rn((float)p.crop_h, (float)out_h), ws = __fdiv_rn((float)p.crop_w, (float)out_w);
    // byte loads through a buffer resource over the frame (< 2^31 bytes): each byte is its own load, whatever the frame's
    // alignment (a plain pointer lets the compiler pair bytes into unaligned 16-bit loads), and a stray index reads 0
    const __amdgpu_buffer_rsrc_t frame = __builtin_amdgcn_make_buffer_rsrc((void *)(images + p.offset), 0, p.height * p.width * 3, 0x00020000);
    const int row = (p.crop_y + nn_src(y, hs, p.crop_h)) * p.width * 3;
    float v[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = row + (p.crop_x + nn_src(x + i, ws, p.crop_w)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = (float)__builtin_amdgcn_raw_buffer_load_b8(frame, px, c, 0) * (float)(1.0 / 255.0);
    }
    if (p.flags & SSD_AUG_COLOR) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[i][c] = clip01(v[i][c] + p.color_offset[c]);
    }
    if (p.flags & SSD_AUG_GRAY) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float g = (v[i][0] * 0.2989f + v[i][1] * 0.5870f) + v[i][2] * 0.1140f;
            v[i][0] = g; v[i][1] = g; v[i][2] = g;
        }
    }
    if (p.flags & SSD_AUG_SCALE) {
        const uint32_t k0 = (uint32_t)p.philox_key, k1 = (uint32_t)(p.philox_key >> 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t r[4];
            philox4x32_10((uint32_t)y * (uint32_t)out_w + (uint32_t)(x + i), k0, k1, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float f = uint_to_unit(r[c]) * p.scale_range + p.scale_min;
                v[i][c] = clip01(v[i][c] * f);
            }
        }
    }
    int xo = x;
    if (p.flags & SSD_AUG_FLIP) {
        xo = out_w - 4 - x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = v[0][c]; v[0][c] = v[3][c]; v[3][c] = t;
            t = v[1][c]; v[1][c] = v[2][c]; v[2][c] = t;
        }
    }
    const int64_t plane = (int64_t)out_h * out_w;
    if (channels_first) {
        float *o = out + (int64_t)b * 3 * plane + (int64_t)y * out_w + xo;
#pragma unroll
        for (int c = 0; c < 3; ++c) *(v4f *)(o + c * plane) = v4f{v[0][c], v[1][c], v[2][c], v[3][c]};
    } else {
        v4f *o = (v4f *)(out + ((int64_t)b * plane + (int64_t)y * out_w + xo) * 3);
        o[0] = v4f{v[0][0], v[0][1], v[0][2], v[1][0]};
        o[1] = v4f{v[1][1], v[1][2], v[2][0], v[2][1]};
        o[2] = v4f{v[2][2], v[3][0], v[3][1], v[3][2]};
    }
}

}  // namespace

extern "C" int ssd_augment(const uint8_t *images_dev, const ssd_augment_params *params_host, const ssd_augment_params *params_dev,
                           int32_t B, int32_t out_h, int32_t out_w, int32_t channels_first, float *out_dev, void *stream)
{
    if (!images_dev || !params_host || !params_dev || !out_dev || B < 1)
        return ssd_fail(SSD_ERR_INVALID, "ssd_augment: bad arguments");
    if (out_h < 128 || out_w < 128 || out_h % 128 || out_w % 128)
        return ssd_fail(SSD_ERR_INVALID, "ssd_augment: out_h and out_w must be positive multiples of 128");
    if ((uintptr_t)out_dev & 15) return ssd_fail(SSD_ERR_INVALID, "ssd_augment: out must be 16-byte aligned");
    if ((uintptr_t)params_dev & 7) return ssd_fail(SSD_ERR_INVALID, "ssd_augment: params_dev must be 8-byte aligned");
    const int64_t per_image = (int64_t)out_h * out_w;
    if (per_image > INT_MAX) return ssd_fail(SSD_ERR_INVALID, "ssd_augment: out_h * out_w must stay below 2^31");
    const int64_t blocks_per_image = per_image / AUG_PIXELS;             // exact: out_h * out_w is a multiple of 16 384
    if (blocks_per_image > INT_MAX / B) return ssd_fail(SSD_ERR_INVALID, "ssd_augment: batch too large");
    for (int32_t b = 0; b < B; ++b) {
        const ssd_augment_params &p = params_host[b];
        if (p.height < 1 || p.width < 1 || p.offset < 0 || (int64_t)p.height * p.width * 3 > INT_MAX || p.offset > ((int64_t)1 << 60))
            return ssd_fail(SSD_ERR_INVALID, "ssd_augment: image " + std::to_string(b) + ": bad frame");
        if (p.crop_h < 1 || p.crop_w < 1 || p.crop_y < 0 || p.crop_x < 0 || p.crop_y > p.height - p.crop_h ||
            p.crop_x > p.width - p.crop_w)
            return ssd_fail(SSD_ERR_INVALID, "ssd_augment: image " + std::to_string(b) + ": empty or out-of-frame crop window");
        if (p.flags & ~AUG_FLAGS) return ssd_fail(SSD_ERR_INVALID, "ssd_augment: image " + std::to_string(b) + ": unknown flags");
    }
    hipLaunchKernelGGL(augment, dim3((unsigned)(blocks_per_image * B)), dim3(AUG_THREADS), 0, (hipStream_t)stream, images_dev,
                       params_dev, out_h, out_w, (int)blocks_per_image, channels_first ? 1 : 0, out_dev);
    HIPCHK(hipGetLastError());
    return SSD_OK;
}
