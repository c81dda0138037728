// The geometry an accepted JPEG stream gives (include/ssd_hip.h, block "the JPEG decoder"), as the host stage's plan and the
// device stage's table check both test it, and the zigzag order both host stages (jpeg_host.cpp, jpeg_emit.cpp) code in.
// Plain C++: the host stages include no HIP header.
#pragma once
#include <stdint.h>

// position k of the zigzag sequence -> index in natural (row-major) order
static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

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
