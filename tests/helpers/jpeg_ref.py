"""The JPEG decoder's rules restated in numpy, written from include/ssd_hip.h (block "the JPEG decoder") and not from the kernels:
a small marker parser and Huffman decoder in plain Python (one bit at a time: for the small files of the tests), and the
dequantisation, the inverse DCT, the chroma upsampling and the colour conversion as array arithmetic in int64 wrapped to int32.

    parse(blob)  -> dict(height, width, components, h, v, mcus_x, mcus_y, restart, coef [int16 per component: blocks x 64],
                         quant [uint16 components x 64])
    pixels(p)    -> uint8 [height, width, 3]
    ranges(p)    -> (max |x|, max |pass-1 output|, min v, max v) of both passes in exact integers, nothing wrapped
    pinned(p)    -> the header's rule for "PIL's frame is pinned": what ssd_jpeg_entropy accepts"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            c = self.d[self.p]
            if c == 0xFF:
                assert self.d[self.p + 1] == 0, "a marker inside the entropy data"
                self.p += 2
            else:
                self.p += 1
            self.acc, self.n = c, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, m):
        self.n = 0
        while self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xFF:
            self.p += 1
        assert self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + m, "restart marker"
        self.p += 2


def _codes(counts, symbols):
    """{(length, code): symbol} of a DHT table."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise AssertionError("no such Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def parse(blob):
    d = bytes(blob)
    assert d[:2] == b"\xff\xd8"
    p, quant, dc, ac, restart, frame = 2, {}, {}, {}, 0, None
    while True:
        assert d[p] == 0xFF
        while d[p] == 0xFF:
            p += 1
        m, length = d[p], (d[p + 1] << 8) | d[p + 2]
        seg, p = d[p + 3:p + 1 + length], p + 1 + length
        if m == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = np.frombuffer(seg[1:65], np.uint8)
                quant[seg[0] & 15], seg = q, seg[65:]
        elif m == 0xC4:
            while seg:
                counts = list(seg[1:17])
                total = sum(counts)
                (ac if seg[0] >> 4 else dc)[seg[0] & 15] = _codes(counts, list(seg[17:17 + total]))
                seg = seg[17 + total:]
        elif m == 0xDD:
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xC0:
            assert seg[0] == 8
            frame = {"height": (seg[1] << 8) | seg[2], "width": (seg[3] << 8) | seg[4],
                     "comps": [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]}
        elif m == 0xDA:
            assert frame is not None and seg[0] == len(frame["comps"])
            tables = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            break
        else:
            assert m >= 0xE0 or m == 0xFE, "marker %02x" % m
    comps = frame["comps"]
    n = len(comps)
    h, v = comps[0][1], comps[0][2]
    H, W = frame["height"], frame["width"]
    mcus_x, mcus_y = -(-W // (8 * h)), -(-H // (8 * v))
    hs, vs = [h] + [1] * (n - 1), [v] + [1] * (n - 1)
    coef = [np.zeros((mcus_y * vs[c] * mcus_x * hs[c], 64), np.int16) for c in range(n)]
    br, pred, count, rst = _Bits(d, p), [0] * n, 0, 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if restart and count and count % restart == 0:
                br.restart(rst)
                rst, pred = (rst + 1) & 7, [0] * n
            for c in range(n):
                for vy in range(vs[c]):
                    for hx in range(hs[c]):
                        block = coef[c][(my * vs[c] + vy) * (mcus_x * hs[c]) + mx * hs[c] + hx]
                        s = _symbol(br, dc[tables[c][0]])
                        if s:
                            pred[c] += _extend(br.bits(s), s)
                        block[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = _symbol(br, ac[tables[c][1]])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            block[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
            count += 1
    return {"height": H, "width": W, "components": n, "h": h, "v": v, "mcus_x": mcus_x, "mcus_y": mcus_y, "restart": restart,
            "coef": coef, "quant": np.stack([quant[comps[c][3]] for c in range(n)])}


# ----------------------------------------------------------------------------- the arithmetic
def _i32(x):
    """int64 values wrapped to 32-bit two's complement."""
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _exact(x):
    return np.asarray(x, np.int64)


def _idct_1d(x, _i32=_i32):
    """The one-dimensional kernel over the LAST axis (8 values) -> the eight outputs before descaling; `_i32` is the wrap of
    every sum (ranges() passes none: int64 holds every exact value of 8-bit tables on int16 coefficients)."""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = _i32((x2 + x6) * 4433)
    t2, t3 = _i32(z1 - x6 * 15137), _i32(z1 + x2 * 6270)
    t0, t1 = _i32((x0 + x4) << 13), _i32((x0 - x4) << 13)
    t10, t13, t11, t12 = _i32(t0 + t3), _i32(t0 - t3), _i32(t1 + t2), _i32(t1 - t2)
    a, b, c, d = x7, x5, x3, x1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = _i32((z3 + z4) * 9633)
    a, b, c, d = _i32(a * 2446), _i32(b * 16819), _i32(c * 25172), _i32(d * 12299)
    z1, z2 = _i32(z1 * -7373), _i32(z2 * -20995)
    z3, z4 = _i32(z3 * -16069 + z5), _i32(z4 * -3196 + z5)
    a, b, c, d = _i32(a + z1 + z3), _i32(b + z2 + z4), _i32(c + z2 + z3), _i32(d + z1 + z4)
    return np.stack([_i32(t10 + d), _i32(t11 + c), _i32(t12 + b), _i32(t13 + a),
                     _i32(t13 - a), _i32(t12 - b), _i32(t11 - c), _i32(t10 - d)], -1)


def idct_blocks(coef, q):
    """coef int16 [n, 64], q uint16 [64] -> uint8 [n, 8, 8]."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    cols = _i32(_idct_1d(x.transpose(0, 2, 1)) + (1 << 10)) >> 11           # [n, column, output row]
    ws = cols.transpose(0, 2, 1)                                            # [n, row, column]
    rows = _i32(_idct_1d(ws) + (1 << 17)) >> 18
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


X_LIMIT, W_LIMIT, V_MIN, V_MAX = 16383, 16383, -512, 511           # the header's three limbs


def block_ranges(coef, q):
    """Per block of coef int [n, 64] under the table q [64]: (max |x|, max |w|, min v, max v), int64 [n] each -- x the dequantised
    values, w pass 1's descaled outputs, v pass 2's descaled outputs before + 128: the header's two passes in exact integers,
    nothing wrapped."""
    x = (np.asarray(coef, np.int64).reshape(-1, 64) * np.asarray(q, np.int64).reshape(64)).reshape(-1, 8, 8)
    assert int(np.abs(x).max(initial=0)) < 1 << 24, "exact in int64 for 8-bit tables on int16 coefficients"
    ws = ((_idct_1d(x.transpose(0, 2, 1), _exact) + (1 << 10)) >> 11).transpose(0, 2, 1)
    v = ((_idct_1d(ws, _exact) + (1 << 17)) >> 18).reshape(-1, 64)
    return np.abs(x).reshape(-1, 64).max(1), np.abs(ws).reshape(-1, 64).max(1), v.min(1), v.max(1)


def blocks_pinned(coef, q):
    """bool [n]: the header's three limbs, block by block."""
    ax, aw, lo, hi = block_ranges(coef, q)
    return (ax <= X_LIMIT) & (aw <= W_LIMIT) & (lo >= V_MIN) & (hi <= V_MAX)


def ranges(p):
    """(max |x|, max |w|, min v, max v) over every block of every component of a parsed file."""
    parts = [block_ranges(coef, q) for coef, q in zip(p["coef"], p["quant"])]
    return (max(int(a.max()) for a, _w, _l, _h in parts), max(int(w.max()) for _a, w, _l, _h in parts),
            min(int(lo.min()) for _a, _w, lo, _h in parts), max(int(hi.max()) for _a, _w, _l, hi in parts))


def pinned(p):
    """The header's rule "pinned streams": what ssd_jpeg_entropy accepts of the streams its parser takes."""
    return all(bool(blocks_pinned(coef, q).all()) for coef, q in zip(p["coef"], p["quant"]))


def plane(coef, q, blocks_y, blocks_x):
    """A component's padded sample plane uint8 [8 * blocks_y, 8 * blocks_x]."""
    b = idct_blocks(coef, q).reshape(blocks_y, blocks_x, 8, 8)
    return b.transpose(0, 2, 1, 3).reshape(8 * blocks_y, 8 * blocks_x)


def upsample_h2v1(s, W):
    """s int [rows, n] real samples -> [rows, 2n] cropped to W."""
    s = s.astype(np.int64)
    n = s.shape[1]
    if n <= 2:
        return np.repeat(s, 2, 1)[:, :W]
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * n), np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out[:, :W]


def upsample_h2v2(s, H, W):
    """s int [m, n] real samples -> [2m, 2n] cropped to H x W."""
    s = s.astype(np.int64)
    m, n = s.shape
    if n <= 2:
        return np.repeat(np.repeat(s, 2, 0), 2, 1)[:H, :W]
    up, down = np.concatenate([s[:1], s[:-1]], 0), np.concatenate([s[1:], s[-1:]], 0)
    out = np.empty((2 * m, 2 * n), np.int64)
    for v, nb in ((0, up), (1, down)):
        c = 3 * s + nb
        left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
        even, odd = (3 * c + left + 8) >> 4, (3 * c + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out[:H, :W]


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pixels(p):
    H, W, h, v = p["height"], p["width"], p["h"], p["v"]
    y = plane(p["coef"][0], p["quant"][0], p["mcus_y"] * v, p["mcus_x"] * h)[:H, :W]
    if p["components"] == 1:
        return np.repeat(y[:, :, None], 3, 2)
    n, m = -(-W // 2), -(-H // 2)
    chroma = []
    for c in (1, 2):
        s = plane(p["coef"][c], p["quant"][c], p["mcus_y"], p["mcus_x"])
        if (h, v) == (1, 1):
            chroma.append(s[:H, :W])
        elif (h, v) == (2, 1):
            chroma.append(upsample_h2v1(s[:H, :n], W))
        else:
            chroma.append(upsample_h2v2(s[:m, :n], H, W))
    return colour(y, chroma[0], chroma[1])
