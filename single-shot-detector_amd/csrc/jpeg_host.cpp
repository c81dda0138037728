// The JPEG decoder's host stage: the marker structure, the Huffman decoding and the batch layout.  Plain C++ without a HIP include,
// so that it also compiles and links on its own (tests/jpeg_host_check.cpp runs it under the address and undefined-behaviour
// sanitizers).  What is accepted, what is refused and the coefficient layout: include/ssd_hip.h, block "the JPEG decoder".
//
// No global state beyond constant tables; every entry point works on its arguments and its own stack, so the callers' threads run
// it in parallel.  Every read of the stream goes through a bound check against `n`; every write lands inside the sizes of `info`,
// which ssd_jpeg_entropy re-derives from the bytes and compares before it writes anything.
//
// Huffman decoding: a 64-bit bit buffer, filled a byte at a time with the FF 00 stuffing removed and stopped at any marker, and per
// table a lookahead over the next LOOK (9) bits -- symbol and length of every code of up to 9 bits -- with the canonical
// maxcode / valptr walk for the longer ones.
#include "../../include/ssd_hip.h"
#include "jpeg_geom.h"

#include <cstring>
#include <new>

namespace {

constexpr int LOOK = 9;

struct Huff {
    bool defined = false;
    uint8_t bits[17];           // codes of each length 1 .. 16
    uint8_t vals[256];
    int nvals = 0;
    int32_t maxcode[18];        // largest code of each length, -1: none
    int32_t valptr[17], mincode[17];
    uint16_t look[1 << LOOK];   // (length << 8) | symbol for every LOOK-bit window that starts with a code of <= LOOK bits, else 0
};

struct Header {
    int height = 0, width = 0, ncomp = 0;
    int id[3] = {0, 0, 0}, h[3] = {0, 0, 0}, v[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint16_t quant[4][64];
    bool have_q[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart = 0;
    bool jfif = false, adobe = false;
    int adobe_transform = -1;
    int64_t scan_begin = 0;     // first byte of the entropy-coded data
};

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// the canonical code of a DHT segment's counts and symbols -> decoding tables; false: over-subscribed
bool build_huff(Huff &t)
{
    int32_t code = 0;
    int k = 0;
    for (int i = 0; i < (1 << LOOK); ++i) t.look[i] = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        for (int i = 0; i < t.bits[l]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;
            if (l <= LOOK) {
                const int first = code << (LOOK - l), count = 1 << (LOOK - l);
                for (int j = 0; j < count; ++j) t.look[first + j] = (uint16_t)((l << 8) | t.vals[k]);
            }
        }
        t.maxcode[l] = t.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    return true;
}

// Reads every segment up to the scan header, then walks the entropy-coded data to EOI.  SSD_OK, SSD_ERR_UNSUPPORTED or SSD_ERR_INVALID.
int parse(const uint8_t *b, int64_t n, Header &hd)
{
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return SSD_ERR_INVALID;
    int64_t p = 2;
    bool have_sof = false;
    for (;;) {
        // a marker: FF, any number of fill FFs, the code
        if (p >= n || b[p] != 0xFF) return SSD_ERR_INVALID;
        while (p < n && b[p] == 0xFF) ++p;
        if (p >= n) return SSD_ERR_INVALID;
        const int m = b[p++];
        if (m == 0x00 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) return SSD_ERR_INVALID;
        if (p + 2 > n) return SSD_ERR_INVALID;
        const int len = be16(b + p);
        if (len < 2 || p + len > n) return SSD_ERR_INVALID;
        const uint8_t *s = b + p + 2;
        const int sl = len - 2;
        if (m == 0xC0) {
            if (have_sof) return SSD_ERR_INVALID;
            if (sl < 6) return SSD_ERR_INVALID;
            if (s[0] != 8) return SSD_ERR_UNSUPPORTED;
            hd.height = be16(s + 1);
            hd.width = be16(s + 3);
            const int nf = s[5];
            if (sl != 6 + 3 * nf) return SSD_ERR_INVALID;
            if (hd.width == 0 || nf == 0) return SSD_ERR_INVALID;
            if (hd.height == 0) return SSD_ERR_UNSUPPORTED;          // the height comes in a DNL segment
            if (nf != 1 && nf != 3) return SSD_ERR_UNSUPPORTED;
            hd.ncomp = nf;
            for (int c = 0; c < nf; ++c) {
                hd.id[c] = s[6 + 3 * c];
                hd.h[c] = s[7 + 3 * c] >> 4;
                hd.v[c] = s[7 + 3 * c] & 15;
                hd.tq[c] = s[8 + 3 * c];
                if (hd.h[c] < 1 || hd.h[c] > 4 || hd.v[c] < 1 || hd.v[c] > 4 || hd.tq[c] > 3) return SSD_ERR_INVALID;
            }
            if (nf == 1) {
                if (hd.h[0] != 1 || hd.v[0] != 1) return SSD_ERR_UNSUPPORTED;
            } else {
                if (hd.h[1] != 1 || hd.v[1] != 1 || hd.h[2] != 1 || hd.v[2] != 1) return SSD_ERR_UNSUPPORTED;
                const bool ok = (hd.h[0] == 1 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 2);
                if (!ok) return SSD_ERR_UNSUPPORTED;
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            return SSD_ERR_UNSUPPORTED;                              // every other frame type, JPG, DAC (arithmetic coding)
        } else if (m == 0xC4) {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) return SSD_ERR_INVALID;
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return SSD_ERR_INVALID;
                Huff &t = tc ? hd.ac[th] : hd.dc[th];
                int total = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (t.bits[l] = s[q + l]);
                if (total > 256 || q + 17 + total > sl) return SSD_ERR_INVALID;
                memcpy(t.vals, s + q + 17, (size_t)total);
                t.nvals = total;
                if (!build_huff(t)) return SSD_ERR_INVALID;
                t.defined = true;
                q += 17 + total;
            }
        } else if (m == 0xDB) {
            int q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return SSD_ERR_INVALID;
                if (pq == 1) return SSD_ERR_UNSUPPORTED;
                if (q + 65 > sl) return SSD_ERR_INVALID;
                for (int k = 0; k < 64; ++k) hd.quant[tq][ZIGZAG[k]] = s[q + 1 + k];
                hd.have_q[tq] = true;
                q += 65;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return SSD_ERR_INVALID;
            hd.restart = be16(s);
        } else if (m == 0xDC) {
            return SSD_ERR_UNSUPPORTED;                              // DNL
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) hd.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
                hd.adobe = true;
                hd.adobe_transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!have_sof) return SSD_ERR_INVALID;
            if (sl < 1) return SSD_ERR_INVALID;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return SSD_ERR_INVALID;
            if (ns != hd.ncomp) return SSD_ERR_UNSUPPORTED;          // a scan of some components: more scans follow
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != hd.id[c]) return SSD_ERR_UNSUPPORTED;
                hd.td[c] = s[2 + 2 * c] >> 4;
                hd.ta[c] = s[2 + 2 * c] & 15;
                if (hd.td[c] > 3 || hd.ta[c] > 3) return SSD_ERR_INVALID;
                if (!hd.dc[hd.td[c]].defined || !hd.ac[hd.ta[c]].defined || !hd.have_q[hd.tq[c]]) return SSD_ERR_INVALID;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return SSD_ERR_UNSUPPORTED;
            if (hd.ncomp == 3) {
                bool ycc;
                if (hd.jfif) ycc = true;
                else if (hd.adobe) ycc = hd.adobe_transform == 1;
                else ycc = !(hd.id[0] == 'R' && hd.id[1] == 'G' && hd.id[2] == 'B');
                if (!ycc) return SSD_ERR_UNSUPPORTED;
            }
            p += len;
            hd.scan_begin = p;
            break;
        }
        // APPn, COM and everything unknown with a length: skipped
        p += len;
    }
    // the scan's extent: stuffed bytes and restart markers belong to it; EOI ends the image; anything else is not one scan
    for (;;) {
        const uint8_t *f = (const uint8_t *)memchr(b + p, 0xFF, (size_t)(n - p));
        if (!f) return SSD_ERR_INVALID;
        p = (f - b) + 1;
        while (p < n && b[p] == 0xFF) ++p;
        if (p >= n) return SSD_ERR_INVALID;
        const int m = b[p++];
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return SSD_OK;
        if (m == 0xDA || m == 0xDC || (m >= 0xC0 && m <= 0xCF && m != 0xC4)) return SSD_ERR_UNSUPPORTED;
        if (m == 0xD8 || m == 0x01) return SSD_ERR_INVALID;
        if (p + 2 > n) return SSD_ERR_INVALID;                       // a segment behind the scan (tables, comments): skipped
        const int len = be16(b + p);
        if (len < 2 || p + len > n) return SSD_ERR_INVALID;
        p += len;
    }
}

void fill_info(const Header &hd, ssd_jpeg_info *o)
{
    memset(o, 0, sizeof(*o));
    o->height = hd.height;
    o->width = hd.width;
    o->components = hd.ncomp;
    o->h = hd.h[0];
    o->v = hd.v[0];
    o->mcus_x = (hd.width + 8 * hd.h[0] - 1) / (8 * hd.h[0]);
    o->mcus_y = (hd.height + 8 * hd.v[0] - 1) / (8 * hd.v[0]);
    o->restart_interval = hd.restart;
    const int64_t mcus = (int64_t)o->mcus_x * o->mcus_y;             // <= 8192 * 8192
    o->blocks[0] = (int32_t)(mcus * hd.h[0] * hd.v[0]);
    if (hd.ncomp == 3) o->blocks[1] = o->blocks[2] = (int32_t)mcus;
    o->coef_count = 64 * ((int64_t)o->blocks[0] + o->blocks[1] + o->blocks[2]);
}

// an info an accepted stream gives: the shared geometry, and the counts that follow from it
bool info_ok(const ssd_jpeg_info &f)
{
    if (!jpeg_geometry_ok(f.height, f.width, f.components, f.h, f.v, f.mcus_x, f.mcus_y)) return false;
    const int64_t luma = jpeg_luma_blocks(f.h, f.v, f.mcus_x, f.mcus_y), chroma = jpeg_chroma_blocks(f.components, f.mcus_x, f.mcus_y);
    if (f.blocks[0] != luma || f.blocks[1] != chroma || f.blocks[2] != chroma) return false;
    return f.coef_count == 64 * (luma + 2 * chroma) && f.restart_interval >= 0;
}

// ----------------------------------------------------------------------------- the bit reader
struct Bits {
    const uint8_t *p, *end;
    uint64_t buf = 0;           // the next bits from bit 63 down; zero below `cnt`
    int cnt = 0;
    void fill()
    {
        while (cnt <= 56) {
            if (p >= end) return;
            const unsigned c = *p;
            if (c == 0xFF) {
                if (p + 1 >= end || p[1] != 0x00) return;           // a marker (or the end): the data stops here
                p += 2;
            } else {
                ++p;
            }
            buf |= (uint64_t)c << (56 - cnt);
            cnt += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }      // 1 <= k <= 16; zeros past the data
    void drop(int k)
    {
        buf <<= k;
        cnt -= k;
    }
};

// the next symbol of table t, or -1: no such code / the data ended inside it
inline int decode_symbol(Bits &br, const Huff &t)
{
    if (br.cnt < 16) br.fill();
    const unsigned e = t.look[br.peek(LOOK)];
    if (e) {
        const int l = (int)(e >> 8);
        if (l > br.cnt) return -1;
        br.drop(l);
        return (int)(e & 255);
    }
    const int32_t code16 = (int32_t)br.peek(16);
    for (int l = LOOK + 1; l <= 16; ++l) {
        const int32_t code = code16 >> (16 - l);
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) {
            if (l > br.cnt) return -1;
            const int at = t.valptr[l] + (code - t.mincode[l]);
            if (at >= t.nvals) return -1;
            br.drop(l);
            return t.vals[at];
        }
    }
    return -1;
}

// `s` further bits as the signed value of category s (1 <= s <= 15): false when the data ended
inline bool receive_extend(Bits &br, int s, int &out)
{
    if (br.cnt < s) {
        br.fill();
        if (br.cnt < s) return false;
    }
    const int v = (int)br.peek(s);
    br.drop(s);
    out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

// ----------------------------------------------------------------------------- the pinned rule
// include/ssd_hip.h, "Pinned streams": in every block |x| <= 16383, |w| <= 16383 and -512 <= v <= 511, x the dequantised values,
// w pass 1's descaled outputs, v pass 2's before + 128, all in exact integers.
constexpr int X_LIMIT = 16383, W_LIMIT = 16383, V_MIN = -512, V_MAX = 511;

// The screen: a block with S = sum |x| <= SCREEN_SUM holds all three limbs, so only louder blocks pay for the exact passes.
//   The one-dimensional kernel is linear and exact (its roundings are the two descales); written out, output k = sum_j c[k][j] x[j]
//   with max |c[k][j]| = 11363 (x1 into output 0: 12299 - 7373 - 3196 + 9633), so |output| <= 11363 * sum_j |x[j]|.
//   pass 1, column c with S_c = its sum |x|:  |w| <= (11363 S_c + 1024) / 2048 < 5.5484 S_c + 1
//   pass 2, a row holds one w of every column:  sum |w| < 5.5484 S + 8,  |v| <= (11363 (5.5484 S + 8) + 2^17) / 2^18 + 1
//                                                                            < 0.24050 S + 1.85
//   S <= 2047:  |x| <= 2047,  |w| < 11359,  |v| < 494.2 -- inside 16383, 16383 and [-512, 511].
constexpr int SCREEN_SUM = 2047;

// the header's one-dimensional kernel in 64-bit integers (nothing wraps for |x| <= X_LIMIT, nor for |w| <= W_LIMIT); the inputs
// and the outputs stride by `step`
inline void idct_1d_exact(const int64_t *x, int step, int64_t *out)
{
    const int64_t x0 = x[0], x1 = x[step], x2 = x[2 * step], x3 = x[3 * step], x4 = x[4 * step], x5 = x[5 * step], x6 = x[6 * step],
                  x7 = x[7 * step];
    int64_t z1 = (x2 + x6) * 4433;
    const int64_t t2 = z1 - x6 * 15137, t3 = z1 + x2 * 6270;
    const int64_t t0 = (x0 + x4) * 8192, t1 = (x0 - x4) * 8192;
    const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int64_t a = x7, b = x5, c = x3, d = x1;
    z1 = a + d;
    int64_t z2 = b + c, z3 = a + c, z4 = b + d;
    const int64_t z5 = (z3 + z4) * 9633;
    a *= 2446, b *= 16819, c *= 25172, d *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
    out[0] = t10 + d, out[step] = t11 + c, out[2 * step] = t12 + b, out[3 * step] = t13 + a;
    out[4 * step] = t13 - a, out[5 * step] = t12 - b, out[6 * step] = t11 - c, out[7 * step] = t10 - d;
}

// floor(t / 2^s) of a signed value without shifting a negative one
inline int64_t descale(int64_t t, int s)
{
    const int64_t r = t + ((int64_t)1 << (s - 1)), d = (int64_t)1 << s;
    return r >= 0 ? r / d : -((-r + d - 1) / d);
}

// the limbs on w and v of one block by both passes in exact integers; every |coefficient * q| <= X_LIMIT already
bool block_pinned(const int16_t *coef, const uint16_t *q)
{
    int64_t x[64], w[64], v[8];
    for (int i = 0; i < 64; ++i) x[i] = (int64_t)coef[i] * (int64_t)q[i];
    for (int c = 0; c < 8; ++c) {
        idct_1d_exact(x + c, 8, w + c);
        for (int r = 0; r < 8; ++r) {
            const int64_t d = descale(w[8 * r + c], 11);
            if (d > W_LIMIT || d < -W_LIMIT) return false;
            w[8 * r + c] = d;
        }
    }
    for (int r = 0; r < 8; ++r) {
        idct_1d_exact(w + 8 * r, 1, v);
        for (int c = 0; c < 8; ++c) {
            const int64_t d = descale(v[c], 18);
            if (d > V_MAX || d < V_MIN) return false;
        }
    }
    return true;
}

// one block into `dst` (64 zeros on entry): SSD_OK or the refusal
inline int decode_block(Bits &br, const Huff &dc, const Huff &ac, const uint16_t *q, int &pred, int16_t *dst)
{
    const int s = decode_symbol(br, dc);
    if (s < 0 || s > 11) return SSD_ERR_INVALID;
    if (s) {
        int diff;
        if (!receive_extend(br, s, diff)) return SSD_ERR_INVALID;
        pred += diff;                                                // |pred| stays below 2^11 * blocks < 2^31
    }
    if (pred < -32768 || pred > 32767) return SSD_ERR_UNSUPPORTED;
    int sum;                                                         // S = sum |x| of the block: at most 64 * X_LIMIT
    {
        const int prod = pred * (int)q[0];
        if (prod > X_LIMIT || prod < -X_LIMIT) return SSD_ERR_UNSUPPORTED;
        sum = prod < 0 ? -prod : prod;
    }
    dst[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return SSD_ERR_INVALID;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;                                      // end of block
            k += 16;                                                 // sixteen zeros
            continue;
        }
        k += r;
        if (k > 63) return SSD_ERR_INVALID;
        int val;
        if (!receive_extend(br, sz, val)) return SSD_ERR_INVALID;
        const int nat = ZIGZAG[k];
        const int prod = val * (int)q[nat];
        if (prod > X_LIMIT || prod < -X_LIMIT) return SSD_ERR_UNSUPPORTED;
        sum += prod < 0 ? -prod : prod;
        dst[nat] = (int16_t)val;                                     // |val| < 2^15
        ++k;
    }
    if (sum > SCREEN_SUM && !block_pinned(dst, q)) return SSD_ERR_UNSUPPORTED;
    return SSD_OK;
}

}  // namespace

extern "C" int ssd_jpeg_info_read(const uint8_t *bytes, int64_t n, ssd_jpeg_info *out)
{
    if (!bytes || !out || n < 0) return SSD_ERR_INVALID;
    Header *hd = new (std::nothrow) Header();
    if (!hd) return SSD_ERR_INVALID;
    const int rc = parse(bytes, n, *hd);
    if (rc == SSD_OK) fill_info(*hd, out);
    delete hd;
    return rc;
}

extern "C" int ssd_jpeg_entropy(const uint8_t *bytes, int64_t n, const ssd_jpeg_info *info, int16_t *coef_host, uint16_t *quant_host)
{
    if (!bytes || !info || !coef_host || !quant_host || n < 0) return SSD_ERR_INVALID;
    struct Owner {
        Header *hd = new (std::nothrow) Header();
        ~Owner() { delete hd; }
    } own;
    if (!own.hd) return SSD_ERR_INVALID;
    Header &hd = *own.hd;
    const int rc = parse(bytes, n, hd);
    if (rc != SSD_OK) return rc;
    ssd_jpeg_info mine;
    fill_info(hd, &mine);
    if (memcmp(&mine, info, sizeof(mine)) != 0) return SSD_ERR_INVALID;     // every write below stays inside what `info` reports

    for (int c = 0; c < hd.ncomp; ++c) memcpy(quant_host + 64 * c, hd.quant[hd.tq[c]], 64 * sizeof(uint16_t));
    memset(coef_host, 0, (size_t)mine.coef_count * sizeof(int16_t));

    int16_t *base[3] = {coef_host, coef_host + 64 * (int64_t)mine.blocks[0], coef_host + 64 * ((int64_t)mine.blocks[0] + mine.blocks[1])};
    const int hs[3] = {hd.h[0], 1, 1}, vs[3] = {hd.v[0], 1, 1};
    Bits br;
    br.p = bytes + hd.scan_begin;
    br.end = bytes + n;
    int pred[3] = {0, 0, 0};
    int until_restart = hd.restart, next_rst = 0;
    const int64_t mcus = (int64_t)mine.mcus_x * mine.mcus_y;
    int64_t done = 0;
    for (int my = 0; my < mine.mcus_y; ++my) {
        for (int mx = 0; mx < mine.mcus_x; ++mx) {
            for (int c = 0; c < hd.ncomp; ++c) {
                const int64_t row_blocks = (int64_t)mine.mcus_x * hs[c];
                for (int vy = 0; vy < vs[c]; ++vy) {
                    for (int hx = 0; hx < hs[c]; ++hx) {
                        const int64_t blk = ((int64_t)my * vs[c] + vy) * row_blocks + (int64_t)mx * hs[c] + hx;
                        const int r = decode_block(br, hd.dc[hd.td[c]], hd.ac[hd.ta[c]], quant_host + 64 * c, pred[c], base[c] + 64 * blk);
                        if (r != SSD_OK) return r;
                    }
                }
            }
            ++done;
            if (hd.restart && --until_restart == 0 && done < mcus) {
                // the padding bits of the interval's last byte go; RSTm, m counting modulo 8, follows (fill FFs in front allowed)
                br.buf = 0;
                br.cnt = 0;
                const uint8_t *p = br.p;
                if (p >= br.end || *p != 0xFF) return SSD_ERR_INVALID;
                while (p < br.end && *p == 0xFF) ++p;
                if (p >= br.end || *p != 0xD0 + next_rst) return SSD_ERR_INVALID;
                br.p = p + 1;
                next_rst = (next_rst + 1) & 7;
                until_restart = hd.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
        }
    }
    return SSD_OK;
}

extern "C" int ssd_jpeg_plan(const ssd_jpeg_info *infos, int32_t B, ssd_jpeg_image *images_out, int64_t *totals_out)
{
    if (B < 0 || B > (1 << 20) || !totals_out || (B > 0 && (!infos || !images_out))) return SSD_ERR_INVALID;
    int64_t coef = 0, quant = 0, plane = 0, frame = 0, blocks = 0, tiles = 0;
    for (int32_t b = 0; b < B; ++b) {
        const ssd_jpeg_info &f = infos[b];
        if (!info_ok(f)) return SSD_ERR_INVALID;
        ssd_jpeg_image &g = images_out[b];
        g.height = f.height, g.width = f.width, g.components = f.components, g.h = f.h, g.v = f.v;
        g.mcus_x = f.mcus_x, g.mcus_y = f.mcus_y, g.reserved = 0;
        g.coef_offset = coef, g.quant_offset = quant, g.plane_offset = plane, g.frame_offset = frame;
        g.block_begin = blocks, g.tile_begin = tiles;
        const int64_t nb = (int64_t)f.blocks[0] + f.blocks[1] + f.blocks[2], px = (int64_t)f.height * f.width;
        coef += 64 * nb;
        quant += 64 * (int64_t)f.components;
        plane += (64 * nb + 15) & ~(int64_t)15;
        blocks += nb;
        tiles += (px + SSD_JPEG_TILE - 1) / SSD_JPEG_TILE;
        if (frame + 3 * px > 0x7fffffffLL) return SSD_ERR_INVALID;
        frame += (3 * px + 15) & ~(int64_t)15;
    }
    totals_out[0] = coef, totals_out[1] = quant, totals_out[2] = plane, totals_out[3] = frame;
    return SSD_OK;
}
