// The JPEG encoder's quality scaling (include/ssd_hip.h, block "the JPEG encoder"), as the host stage writes it into DQT and the
// device stage divides by it: the Annex K.1 base tables in natural order and jpeg_quality_scaling's rule.  Plain C++: jpeg_emit.cpp
// includes no HIP header.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JPEG_QUANT_HD __host__ __device__
#else
#define JPEG_QUANT_HD
#endif

// luma, then chroma
#define JPEG_BASE_Q_INIT                                                                                                                 \
    {{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,    \
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,  \
      103, 99},                                                                                                                          \
     {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,    \
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}}

// quality in 1 .. 100 -> the percentage the base tables are scaled by
JPEG_QUANT_HD static inline int jpeg_quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

// one table entry, 1 .. 255
JPEG_QUANT_HD static inline int jpeg_quant_entry(int base, int scale)
{
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}
