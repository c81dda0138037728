// The JPEG encoder's host stage: the quality scaling, the batch layout, and the whole file of one image from its quantised
// coefficients -- markers, Huffman coding with the Annex K tables, byte stuffing.  Plain C++ without a HIP include, so that it also
// compiles and links on its own (tests/jpeg_emit_check.cpp runs it under the address and undefined-behaviour sanitizers).  The
// rules, the file's order and the coefficient layout: include/ssd_hip.h, block "the JPEG encoder".
//
// No global state beyond constant tables; every entry point works on its arguments and its own stack, so the callers' threads run
// images in parallel.  Every byte goes through Out::put, which compares with the capacity first; dummy blocks are coded by their
// rule and never read.
#include "../../include/ssd_hip.h"
#include "jpeg_geom.h"
#include "jpeg_quant.h"

#include <cstring>

namespace {

const uint8_t BASE_Q[2][64] = JPEG_BASE_Q_INIT;      // Annex K.1, natural order

// Annex K.3: codes of each length 1 .. 16, then the symbols in code order.  Table 0: luma, 1: chroma.
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// SSD_OK and the luma factors of a sampling code, or the refusal
int sampling_factors(int32_t sampling, int &h, int &v)
{
    if (sampling == SSD_JPEG_SAMPLING_444) h = v = 1;
    else if (sampling == SSD_JPEG_SAMPLING_420) h = v = 2;
    else return SSD_ERR_UNSUPPORTED;
    return SSD_OK;
}

int check_geometry(int32_t height, int32_t width, int32_t sampling, int &h, int &v)
{
    const int rc = sampling_factors(sampling, h, v);
    if (rc != SSD_OK) return rc;
    return height >= 1 && height <= 65535 && width >= 1 && width <= 65535 ? SSD_OK : SSD_ERR_INVALID;
}

// code and length of every symbol of a table; length 0: no such symbol
struct Codes {
    uint16_t code[256];
    uint8_t len[256];
};

void build_codes(const uint8_t *bits, const uint8_t *vals, Codes &t)
{
    memset(&t, 0, sizeof(t));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            t.code[vals[k]] = (uint16_t)code;
            t.len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

// the output: bytes inside [p, p + cap) only; `over` once a byte did not fit
struct Out {
    uint8_t *p;
    int64_t cap, n = 0;
    bool over = false;
    uint64_t acc = 0;           // the bits not yet written, in the low `cnt` bits
    int cnt = 0;
    void put(unsigned byte)
    {
        if (n < cap) p[n++] = (uint8_t)byte;
        else over = true;
    }
    void put16(unsigned v) { put(v >> 8), put(v & 255); }
    void bytes(const uint8_t *s, int count)
    {
        for (int i = 0; i < count; ++i) put(s[i]);
    }
    // `len` (1 .. 27) bits of the scan, FF followed by 00
    void bits(unsigned value, int len)
    {
        acc = (acc << len) | (value & ((1u << len) - 1u));
        cnt += len;
        while (cnt >= 8) {
            const unsigned b = (unsigned)(acc >> (cnt - 8)) & 255u;
            put(b);
            if (b == 0xFF) put(0);
            cnt -= 8;
        }
    }
    void flush()
    {
        if (cnt) bits(0x7F, 8 - cnt);
    }
};

inline int category(unsigned magnitude)
{
    int n = 0;
    while (magnitude) ++n, magnitude >>= 1;
    return n;
}

// one real block; false: a value no code of the tables holds (a DC difference past category 11, an AC value past category 10)
inline bool put_block(Out &o, const int16_t *c, const Codes &dc, const Codes &ac, int &pred)
{
    {
        const int diff = (int)c[0] - pred;
        pred = c[0];
        const int s = category((unsigned)(diff < 0 ? -diff : diff));
        if (s > 11) return false;
        o.bits(dc.code[s], dc.len[s]);
        if (s) o.bits((unsigned)(diff < 0 ? diff - 1 : diff), s);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int val = c[ZIGZAG[k]];
        if (val == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) o.bits(ac.code[0xF0], ac.len[0xF0]);
        const int s = category((unsigned)(val < 0 ? -val : val));
        if (s > 10) return false;
        const int sym = (run << 4) | s;
        o.bits(ac.code[sym], ac.len[sym]);
        o.bits((unsigned)(val < 0 ? val - 1 : val), s);
        run = 0;
    }
    if (run) o.bits(ac.code[0x00], ac.len[0x00]);
    return true;
}

void put_dht(Out &o, int cls, int id, const uint8_t *bits, const uint8_t *vals)
{
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    o.put16(0xFFC4);
    o.put16(2 + 1 + 16 + total);
    o.put((cls << 4) | id);
    o.bytes(bits, 16);
    o.bytes(vals, total);
}

}  // namespace

extern "C" int ssd_jpeg_quant_tables(int32_t quality, uint16_t *tables_out)
{
    if (!tables_out || quality < 1 || quality > 100) return SSD_ERR_INVALID;
    const int scale = jpeg_quality_scale(quality);
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) tables_out[64 * t + k] = (uint16_t)jpeg_quant_entry(BASE_Q[t][k], scale);
    return SSD_OK;
}

extern "C" int64_t ssd_jpeg_emit_bound(int32_t height, int32_t width, int32_t sampling)
{
    int h, v;
    const int rc = check_geometry(height, width, sampling, h, v);
    if (rc != SSD_OK) return rc;
    const int32_t mcus_x = (width + 8 * h - 1) / (8 * h), mcus_y = (height + 8 * v - 1) / (8 * v);
    // a block: at most 20 bits of DC and 63 * 26 of AC = 208 bytes, every one of them stuffed; the headers are 623 bytes, EOI 2
    return 1024 + 416 * (jpeg_luma_blocks(h, v, mcus_x, mcus_y) + 2 * jpeg_chroma_blocks(3, mcus_x, mcus_y));
}

extern "C" int ssd_jpeg_emit(const int16_t *coef, int32_t height, int32_t width, int32_t sampling, int32_t quality, uint8_t *out,
                             int64_t capacity, int64_t *size_out)
{
    int h, v;
    const int rc = check_geometry(height, width, sampling, h, v);
    if (rc != SSD_OK) return rc;
    uint16_t quant[128];
    if (!coef || !size_out || capacity < 0 || (capacity > 0 && !out) || ssd_jpeg_quant_tables(quality, quant) != SSD_OK) return SSD_ERR_INVALID;
    *size_out = 0;
    Out o;
    o.p = out, o.cap = capacity;

    static const uint8_t JFIF[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    o.put16(0xFFD8);
    o.bytes(JFIF, 18);
    for (int t = 0; t < 2; ++t) {
        o.put16(0xFFDB);
        o.put16(67);
        o.put(t);
        for (int k = 0; k < 64; ++k) o.put(quant[64 * t + ZIGZAG[k]]);
    }
    o.put16(0xFFC0);
    o.put16(17);
    o.put(8);
    o.put16((unsigned)height);
    o.put16((unsigned)width);
    o.put(3);
    for (int c = 0; c < 3; ++c) {
        o.put(c + 1);
        o.put(c == 0 ? (h << 4) | v : 0x11);
        o.put(c == 0 ? 0 : 1);
    }
    for (int t = 0; t < 2; ++t) {
        put_dht(o, 0, t, DC_BITS[t], DC_VALS);
        put_dht(o, 1, t, AC_BITS[t], AC_VALS[t]);
    }
    o.put16(0xFFDA);
    o.put16(12);
    o.put(3);
    for (int c = 0; c < 3; ++c) {
        o.put(c + 1);
        o.put(c == 0 ? 0x00 : 0x11);
    }
    o.put(0), o.put(63), o.put(0);

    Codes dc[2], ac[2];
    for (int t = 0; t < 2; ++t) {
        build_codes(DC_BITS[t], DC_VALS, dc[t]);
        build_codes(AC_BITS[t], AC_VALS[t], ac[t]);
    }
    const int32_t mcus_x = (width + 8 * h - 1) / (8 * h), mcus_y = (height + 8 * v - 1) / (8 * v);
    const int32_t own_x = (width + 7) / 8, own_y = (height + 7) / 8;         // the luma plane's own whole blocks
    const int64_t luma = jpeg_luma_blocks(h, v, mcus_x, mcus_y), chroma = jpeg_chroma_blocks(3, mcus_x, mcus_y);
    const int16_t *base[3] = {coef, coef + 64 * luma, coef + 64 * (luma + chroma)};
    int pred[3] = {0, 0, 0};
    for (int32_t my = 0; my < mcus_y && !o.over; ++my) {
        for (int32_t mx = 0; mx < mcus_x; ++mx) {
            for (int vy = 0; vy < v; ++vy) {
                for (int hx = 0; hx < h; ++hx) {
                    const int64_t by = (int64_t)my * v + vy, bx = (int64_t)mx * h + hx;
                    if (by >= own_y || bx >= own_x) {
                        // a dummy block: DC difference 0, end of block; the predictor stays
                        o.bits(dc[0].code[0], dc[0].len[0]);
                        o.bits(ac[0].code[0], ac[0].len[0]);
                    } else if (!put_block(o, base[0] + 64 * (by * ((int64_t)mcus_x * h) + bx), dc[0], ac[0], pred[0])) {
                        return SSD_ERR_INVALID;
                    }
                }
            }
            for (int c = 1; c < 3; ++c)
                if (!put_block(o, base[c] + 64 * ((int64_t)my * mcus_x + mx), dc[1], ac[1], pred[c])) return SSD_ERR_INVALID;
        }
    }
    o.flush();
    o.put16(0xFFD9);
    if (o.over) return SSD_ERR_INVALID;
    *size_out = o.n;
    return SSD_OK;
}

extern "C" int ssd_jpeg_encode_plan(const int32_t *frames, int32_t B, ssd_jpeg_encode_image *images_out, int64_t *totals_out)
{
    if (B < 0 || B > (1 << 20) || !totals_out || (B > 0 && (!frames || !images_out))) return SSD_ERR_INVALID;
    int64_t coef = 0, plane = 0, frame = 0, blocks = 0, tiles = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int32_t height = frames[4 * b], width = frames[4 * b + 1], quality = frames[4 * b + 3];
        int h, v;
        const int rc = check_geometry(height, width, frames[4 * b + 2], h, v);
        if (rc != SSD_OK) return rc;
        if (quality < 1 || quality > 100) return SSD_ERR_INVALID;
        ssd_jpeg_encode_image &g = images_out[b];
        g.height = height, g.width = width, g.h = h, g.v = v;
        g.mcus_x = (width + 8 * h - 1) / (8 * h), g.mcus_y = (height + 8 * v - 1) / (8 * v);
        g.quality = quality, g.reserved = 0;
        g.frame_offset = frame, g.plane_offset = plane, g.coef_offset = coef, g.block_begin = blocks, g.tile_begin = tiles;
        const int64_t nb = jpeg_luma_blocks(h, v, g.mcus_x, g.mcus_y) + 2 * jpeg_chroma_blocks(3, g.mcus_x, g.mcus_y);
        const int64_t units = 8 * (int64_t)g.mcus_y * g.mcus_x;
        coef += 64 * nb;
        plane += 64 * nb;                                                    // a multiple of 16 as it is
        blocks += nb;
        tiles += (units + SSD_JPEG_ENC_TILE - 1) / SSD_JPEG_ENC_TILE;
        frame += (3 * (int64_t)height * width + 15) & ~(int64_t)15;
    }
    totals_out[0] = coef, totals_out[1] = plane, totals_out[2] = frame, totals_out[3] = blocks;
    return SSD_OK;
}
