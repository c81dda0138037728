"""A writer of crafted baseline JPEG files for the decoder's tests: any quantised coefficients under any 8-bit tables, so that a
test reaches blocks no encoder produces from pixels (one loud coefficient, flat planes of a chosen value, chroma that alternates
from block to block).

    write(coef, quant, height, width, sampling, restart=0) -> bytes

coef: per component int [blocks, 64] in the decoder's own layout (include/ssd_hip.h, block "the JPEG decoder": natural order, NOT
dequantised, raster order over the component's PADDED block grid) -- what jpeg_ref.parse returns; quant: [components, 64] in natural
order, values 1 .. 255; sampling "gray", "444", "422" or "420"; restart: the restart interval in MCUs.  The file carries a JFIF
APP0, one table per component, SOF0, the four Annex K Huffman tables and one interleaved scan.  ValueError for what baseline with
these tables cannot code: an AC magnitude above 1023, a DC difference above 2047, a table value outside 1 .. 255."""
import struct

import numpy as np

from tests.helpers.jpeg_ref import ZIGZAG, _codes

FACTORS = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}

# Annex K.3: codes of each length 1 .. 16, then the symbols in code order.  Table 0: luma, 1: chroma.
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
_TAIL = [16 * r + s for r in range(16) for s in range(1, 11)]           # every (run, size): the order of the 16-bit codes' tail
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1])
# behind the listed heads the remaining symbols follow in ascending order (that IS Annex K's order of its long codes)
AC_VALS = tuple(head + [s for s in sorted(_TAIL) if s not in head] for head in AC_VALS)
assert all(len(v) == 162 == sum(b) for v, b in zip(AC_VALS, AC_BITS)) and all(sum(b) == 12 for b in DC_BITS)


def _book(bits, vals):
    """{symbol: (length, code)}: jpeg_ref._codes inverted."""
    return {sym: key for key, sym in _codes(bits, vals).items()}


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, length, code):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(8 - self.n, (1 << (8 - self.n)) - 1)                # pad with ones


def _value(w, book, run, v, limit, what):
    """Symbol (run, size) and the size's bits of the signed value v."""
    a = abs(v)
    if a > limit:
        raise ValueError("%s %d: baseline codes at most %d" % (what, v, limit))
    size = a.bit_length()
    w.put(*book[16 * run + size])
    if size:
        w.put(size, v if v > 0 else v + (1 << size) - 1)


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + bytes(body)


def write(coef, quant, height, width, sampling, restart=0):
    h, v = FACTORS[sampling]
    n = 1 if sampling == "gray" else 3
    quant = np.asarray(quant).reshape(n, 64)
    if quant.min() < 1 or quant.max() > 255:
        raise ValueError("an 8-bit table holds 1 .. 255")
    if not (1 <= height <= 65535 and 1 <= width <= 65535 and 0 <= restart <= 65535):
        raise ValueError("height, width or restart")
    mcus_x, mcus_y = -(-width // (8 * h)), -(-height // (8 * v))
    hs, vs = [h] + [1] * (n - 1), [v] + [1] * (n - 1)
    coef = [np.asarray(c).reshape(-1, 64) for c in coef]
    if len(coef) != n or any(len(coef[c]) != mcus_y * vs[c] * mcus_x * hs[c] for c in range(n)):
        raise ValueError("coef must hold every block of every component's padded grid")

    out = bytearray(b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    for c in range(n):
        out += _segment(0xDB, bytes([c]) + bytes(int(quant[c][ZIGZAG[k]]) for k in range(64)))
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, n)
                    + b"".join(bytes([c + 1, (hs[c] << 4) | vs[c], c]) for c in range(n)))
    for t in range(1 if n == 1 else 2):
        out += _segment(0xC4, bytes([t] + DC_BITS[t] + DC_VALS)) + _segment(0xC4, bytes([0x10 | t] + AC_BITS[t] + AC_VALS[t]))
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    out += _segment(0xDA, bytes([n]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(n)) + b"\x00\x3f\x00")

    dc = [_book(DC_BITS[t], DC_VALS) for t in (0, 1)]
    ac = [_book(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    w, pred, count, rst = _Writer(), [0] * n, 0, 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if restart and count and count % restart == 0:
                w.flush()
                w.out += bytes([0xFF, 0xD0 + rst])
                rst, pred = (rst + 1) & 7, [0] * n
            for c in range(n):
                t = 1 if c else 0
                for vy in range(vs[c]):
                    for hx in range(hs[c]):
                        block = [int(x) for x in coef[c][(my * vs[c] + vy) * (mcus_x * hs[c]) + mx * hs[c] + hx]]
                        _value(w, dc[t], 0, block[0] - pred[c], 2047, "DC difference")
                        pred[c] = block[0]
                        run = 0
                        for k in range(1, 64):
                            x = block[ZIGZAG[k]]
                            if x == 0:
                                run += 1
                                continue
                            while run > 15:
                                w.put(*ac[t][0xF0])
                                run -= 16
                            _value(w, ac[t], run, x, 1023, "AC coefficient")
                            run = 0
                        if run:
                            w.put(*ac[t][0x00])
            count += 1
    w.flush()
    return bytes(out + w.out + b"\xff\xd9")
