// What an input pixel of the first layer is and where it comes from when the frames are float32 [B,H,W,3] in the network's own
// size (the TRAIN first convolution from float frames, include/ssd_hip.h): the ONE definition under fc32_forward_kernel and
// fc32_wgrad_partial (train_first_f32.hip).  first_pixels.h is the model: device only, everything inlined, every operation
// separately rounded (-ffp-contract=off).
#pragma once
#include "ssd_internal.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

// The pixel value q(x) = fp32(2 * x - 1) of float x (mobilenet_v1.py:34, shufflenet_v2.py: x = 2.0 * images - 1.0).  2 * x is
// exact, so this is ONE rounding; no clamp and no special case.  For x = fp32(u * inv255) it is first_pixels.h's fc_pixel(u).
static __device__ __forceinline__ float f32_pixel(float x) { return 2.0f * x - 1.0f; }

// Byte address of the 3 pixels x 3 channels under a filter row: image row `row` = b * H + 2 oy + ky of the batch, output column
// cx.  9 contiguous floats from a multiple of 24 bytes: every 8-byte access is aligned.
static __device__ __forceinline__ int f32_row_ad(int row, int W, int cx) { return (row * W + 2 * cx) * 12; }

// The row fetch through a range-checked buffer resource over the batch (32-bit byte offsets: B * H * W * 12 < 2^31): pixels 2 cx
// and 2 cx + 1 as three 8-byte loads, pixel 2 cx + 2 as an 8- and a 4-byte load of its own.  !live (row H: outside) sends all of
// them, !col2 (column W: outside) the third pixel's, out of range: they return 0 without touching memory, and no load that
// carries a value in use ever straddles the end of the batch.  x gets q of what came, in (kx, ci) order: the caller zeroes or
// skips the taps that are outside.
static __device__ __forceinline__ void f32_row_fetch(const __amdgpu_buffer_rsrc_t irsrc, bool live, bool col2, int ad, float (&x)[9])
{
    const int a0 = live ? ad : (int)0x80000000u;
    const int a1 = (live && col2) ? ad + 24 : (int)0x80000000u;
    const v2u p0 = __builtin_amdgcn_raw_buffer_load_b64(irsrc, a0, 0, 0);
    const v2u p1 = __builtin_amdgcn_raw_buffer_load_b64(irsrc, a0 + 8, 0, 0);
    const v2u p2 = __builtin_amdgcn_raw_buffer_load_b64(irsrc, a0 + 16, 0, 0);
    const v2u p3 = __builtin_amdgcn_raw_buffer_load_b64(irsrc, a1, 0, 0);
    const unsigned p4 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a1 + 8, 0, 0);
    const unsigned raw[9] = {p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1], p4};
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = f32_pixel(__uint_as_float(raw[k]));
}
