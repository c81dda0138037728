// The geometry an accepted JPEG stream gives (include/ssd_hip.h, block "the JPEG decoder"), as the host stage's plan and the
// device stage's table check both test it.  Plain C++: jpeg_host.cpp includes no HIP header.
#pragma once
#include <stdint.h>

static inline bool jpeg_geometry_ok(int32_t height, int32_t width, int32_t components, int32_t h, int32_t v, int32_t mcus_x, int32_t mcus_y)
{
    if (height < 1 || height > 65535 || width < 1 || width > 65535) return false;
    if (components != 1 && components != 3) return false;
    const bool s11 = h == 1 && v == 1, s21 = h == 2 && v == 1, s22 = h == 2 && v == 2;
    if (!(s11 || (components == 3 && (s21 || s22)))) return false;
    return mcus_x == (width + 8 * h - 1) / (8 * h) && mcus_y == (height + 8 * v - 1) / (8 * v);
}

// blocks of the luma plane and of each chroma plane (0 for one component)
static inline int64_t jpeg_luma_blocks(int32_t h, int32_t v, int32_t mcus_x, int32_t mcus_y) { return (int64_t)mcus_x * mcus_y * h * v; }
static inline int64_t jpeg_chroma_blocks(int32_t components, int32_t mcus_x, int32_t mcus_y) { return components == 3 ? (int64_t)mcus_x * mcus_y : 0; }
