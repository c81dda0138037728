"""Files at and past the edge of the JPEG decoder's "pinned streams" rule (include/ssd_hip.h, block "the JPEG decoder"), shared by
tests/test_jpeg_loud_host.py and tests/test_gpu_jpeg.py.  Every builder returns [(name, blob, p)], p in jpeg_ref.parse's form
(computed, not parsed back: the host test compares ssd_jpeg_entropy's output with it), built once per process and left unchanged.

    loud()        PIL's files under constant quantisation tables: per table the largest constant whose largest |v| stays inside
                  a band (200, 380, 500), and one constant just past each limb of the rule (v, |w|, |x|)
    fractions()   the 288 files of the finding: constants that put max |coefficient * q| at 1, 0.5, 0.25, 0.1 of 32767
    single()      8 x 8 grayscale files of ONE coefficient at each of the 64 positions, both signs: the largest amplitude the rule
                  pins, and one quantisation step more
    corners()     one 4:4:4 file of flat blocks: (Y, Cb, Cr) over {0, 1, 127, 128, 129, 254, 255}^3
    upsampling()  4:2:2 and 4:2:0 files whose chroma differs from block to block (and, variant "ramp", from sample to sample) by
                  amounts at which the rounding biases of the upsampling decide the result"""
import numpy as np

from tests.helpers import jpeg_cases, jpeg_craft, jpeg_ref

BANDS = (200, 380, 500)
SINGLE_Q = 8                                   # the table value of single(): one step is 8 in x
EDGE = (0, 1, 127, 128, 129, 254, 255)
UP_SIZES = (15, 16, 17, 5, 4, 3)               # 4 and 3: chroma planes of two columns / rows, which the library replicates
_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


# ----------------------------------------------------------------------------- PIL's files under constant tables
def constant_tables(blob, values):
    """The file with every value of its k-th quantisation table replaced by values[k] (PIL writes luma, then chroma)."""
    blob, p, k = bytearray(blob), 2, 0
    while blob[p + 1] != 0xDA:
        n = (blob[p + 2] << 8) | blob[p + 3]
        if blob[p + 1] == 0xDB:
            for q in range(p + 4, p + 2 + n, 65):
                blob[q + 1:q + 65] = bytes([values[k]]) * 64
                k += 1
        p += 2 + n
    assert k == len(values)
    return bytes(blob)


def _retabled(p, values):
    """The parse of constant_tables(blob, values), from the parse p of blob: component 0 reads table 0, the others table 1."""
    out = dict(p)
    out["quant"] = np.stack([np.full(64, values[min(c, 1)], np.uint16) for c in range(p["components"])])
    return out


def _tables_of(p):
    """[[component, ...] per table of a PIL file]."""
    return [[0]] if p["components"] == 1 else [[0], [1, 2]]


def _sweep(p, comps):
    """(max |x|, max |w|, min v, max v), each int64 [255]: the components `comps` of p under the constant tables 1 .. 255."""
    coef = np.concatenate([p["coef"][c] for c in comps]).astype(np.int64)
    qs = np.arange(1, 256, dtype=np.int64)
    parts = jpeg_ref.block_ranges((coef[None] * qs[:, None, None]).reshape(-1, 64), np.ones(64, np.int64))
    ax, aw, lo, hi = [a.reshape(255, -1) for a in parts]
    return ax.max(1), aw.max(1), lo.min(1), hi.max(1)


def _bases():
    """[(name, blob, p)]: PIL's files of three sizes x four samplings x {ramp, noise} at quality 90."""
    def make():
        out = []
        for si, (h, w) in enumerate(((8, 8), (16, 16), (37, 53))):
            for sampling in jpeg_cases.SAMPLINGS:
                for ci, content in enumerate(("ramp", "noise")):
                    blob = jpeg_cases.encode(jpeg_cases.pixels(h, w, content, 300 + 10 * si + ci), sampling, 90)
                    out.append(("%dx%d-%s-%s" % (h, w, sampling, content), blob, jpeg_ref.parse(blob)))
        return out
    return _once("bases", make)


def loud():
    def make():
        out = []
        for name, blob, p in _bases():
            sweeps = [_sweep(p, comps) for comps in _tables_of(p)]
            for band in BANDS:
                # per table the largest constant whose largest |v| stays inside the band
                values = [1 + int(np.flatnonzero(np.maximum(-lo, hi) <= band).max()) for _ax, _aw, lo, hi in sweeps]
                out.append(("loud-%s-v%d" % (name, band), constant_tables(blob, values), _retabled(p, values)))
            if not name.startswith("16x16"):
                continue
            ax, aw, lo, hi = [np.stack(a) for a in zip(*sweeps)]
            past = {"v": ((lo < jpeg_ref.V_MIN) | (hi > jpeg_ref.V_MAX)).any(0), "w": (aw > jpeg_ref.W_LIMIT).any(0),
                    "x": (ax > jpeg_ref.X_LIMIT).any(0)}
            for limb, mask in past.items():
                assert mask.any(), "%s: no constant table passes the limb %s" % (name, limb)
                values = [1 + int(np.flatnonzero(mask).min())] * len(sweeps)          # the smallest constant past this limb
                out.append(("loud-%s-past-%s" % (name, limb), constant_tables(blob, values), _retabled(p, values)))
        return out
    return _once("loud", make)


def fractions():
    def make():
        out = []
        for si, (h, w) in enumerate(((8, 8), (16, 16), (37, 53))):
            for sampling in jpeg_cases.SAMPLINGS:
                for quality in jpeg_cases.QUALITIES:
                    for ci, content in enumerate(("ramp", "noise")):
                        blob = jpeg_cases.encode(jpeg_cases.pixels(h, w, content, 500 + 100 * si + quality + ci), sampling, quality)
                        p = jpeg_ref.parse(blob)
                        peaks = [max(int(np.abs(p["coef"][c].astype(np.int64)).max()) for c in comps) for comps in _tables_of(p)]
                        for fraction in (1.0, 0.5, 0.25, 0.1):
                            values = [min(255, max(1, int(fraction * 32767) // max(peak, 1))) for peak in peaks]
                            out.append(("fraction-%dx%d-%s-q%d-%s-%g" % (h, w, sampling, quality, content, fraction),
                                        constant_tables(blob, values), _retabled(p, values)))
        assert len(out) == 288
        return out
    return _once("fractions", make)


# ----------------------------------------------------------------------------- crafted files
def _crafted(name, coef, quant, height, width, sampling):
    coef = [np.asarray(c, np.int16).reshape(-1, 64) for c in coef]
    quant = np.asarray(quant, np.uint16).reshape(len(coef), 64)
    h, v = jpeg_craft.FACTORS[sampling]
    p = {"height": height, "width": width, "components": len(coef), "h": h, "v": v, "mcus_x": -(-width // (8 * h)),
         "mcus_y": -(-height // (8 * v)), "restart": 0, "coef": coef, "quant": quant}
    return name, jpeg_craft.write(coef, quant, height, width, sampling), p


def single():
    """The last amplitude the rule pins and the first it does not, by search over every codable amplitude with block_ranges."""
    def make():
        out, q = [], np.full(64, SINGLE_Q, np.uint16)
        for k in range(64):
            for sign in (1, -1):
                top = 2047 if k == 0 else 1023                               # what baseline codes
                blocks = np.zeros((top, 64), np.int64)
                blocks[:, k] = sign * np.arange(1, top + 1)
                ok = jpeg_ref.blocks_pinned(blocks, q)
                last = int(np.flatnonzero(ok).max())
                assert ok[:last + 1].all() and last + 1 < top, "position %d: the pinned amplitudes are 1 .. some limit" % k
                for row, kind in ((last, "last"), (last + 1, "past")):
                    out.append(_crafted("single-%02d%s-%s" % (k, "+-"[sign < 0], kind), [blocks[row]], q, 8, 8, "gray"))
        return out
    return _once("single", make)


def _flat(value):
    """The block whose samples are all `value` under a table of ones: x0 = 8 (value - 128), w = 4 x0, v = (x0 + 4) >> 3."""
    block = np.zeros(64, np.int16)
    block[0] = 8 * (int(value) - 128)
    return block


def corners():
    def make():
        triples = [(y, cb, cr) for y in EDGE for cb in EDGE for cr in EDGE]
        coef = [np.stack([_flat(t[c]) for t in triples]) for c in range(3)]          # 343 blocks = 7 rows of 49
        return [_crafted("corners", coef, np.ones((3, 64), np.uint16), 56, 392, "444")]
    return _once("corners", make)


# (a, b) with b - a = 2 mod 4: between a block of a and a block of b, 3a + b = 4a + (b - a) lies half way between two multiples of
# 4, so 2x1's + 1 / + 2 decide; 2x2's sums 3c + c' are 4 times that, half way between two multiples of 16: + 8 / + 7 decide
PAIRS = ((100, 102), (37, 43), (0, 254), (255, 1), (129, 127), (200, 90))


def upsampling():
    def make():
        out, n = [], 0
        for sampling in ("422", "420"):
            h, v = jpeg_craft.FACTORS[sampling]
            for height in UP_SIZES:
                for width in UP_SIZES:
                    mx, my = -(-width // (8 * h)), -(-height // (8 * v))
                    for variant in ("flat", "ramp"):
                        luma = np.stack([_flat(90 + 70 * ((i // (mx * h) + i % (mx * h)) % 2)) for i in range(my * v * mx * h)])
                        chroma = []
                        for c in (0, 1):
                            a, b = PAIRS[(n + 3 * c) % len(PAIRS)]
                            blocks = np.stack([_flat(a if (i // mx + i % mx) % 2 == 0 else b) for i in range(my * mx)])
                            if variant == "ramp":                  # the first horizontal and vertical frequency: every sample differs
                                blocks[:, 1], blocks[:, 8] = (-1) ** c * 200, 120
                                blocks[:, 0] = np.clip(blocks[:, 0], -700, 700)
                            chroma.append(blocks)
                        out.append(_crafted("up-%s-%dx%d-%s" % (sampling, height, width, variant), [luma] + chroma,
                                            np.ones((3, 64), np.uint16), height, width, sampling))
                        n += 1
        return out
    return _once("upsampling", make)
