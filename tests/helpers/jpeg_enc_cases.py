"""The JPEG encoder's shared case list: frames made at test time and the files PIL writes from them (nothing is committed) -- the
yardstick every route must reproduce byte for byte, Image.save(format="jpeg", quality=, subsampling=).

216 frames: the 12 sizes of jpeg_cases.SIZES x {noise, smooth, R = G = B} x quality {30, 75, 100} x sampling {4:2:0, 4:4:4}."""
import struct

import numpy as np

from tests.helpers import jpeg_cases, jpeg_ref

CONTENTS = ("noise", "smooth", "gray")
QUALITIES = (30, 75, 100)
SAMPLINGS = ("420", "444")
CODE = {"420": 420, "444": 444}


def frame(h, w, content, seed):
    """uint8 [h, w, 3]: uniform noise, jpeg_cases' ramp, or one noisy ramp channel three times (a grayscale file's frame)."""
    if content == "noise":
        return jpeg_cases.pixels(h, w, "noise", seed)
    arr = jpeg_cases.pixels(h, w, "ramp", seed)
    return arr if content == "smooth" else np.ascontiguousarray(np.repeat(arr[:, :, 2:3], 3, 2))


_cache = {}


def cases():
    """[(name, frame uint8 [H, W, 3], quality, sampling, PIL's bytes)] -- built once per process, left unchanged."""
    if "list" not in _cache:
        out = []
        for si, (h, w) in enumerate(jpeg_cases.SIZES):
            for ci, content in enumerate(CONTENTS):
                for quality in QUALITIES:
                    for sampling in SAMPLINGS:
                        arr = frame(h, w, content, 100 * si + 10 * ci + quality)
                        arr.setflags(write=False)
                        out.append(("%dx%d-%s-q%d-%s" % (h, w, content, quality, sampling), arr, quality, sampling,
                                    jpeg_cases.encode(arr, sampling, quality)))
        assert len(out) == 216
        _cache["list"] = out
    return _cache["list"]


def parsed():
    """jpeg_ref.parse of every case's PIL file, once."""
    if "parsed" not in _cache:
        _cache["parsed"] = [jpeg_ref.parse(c[4]) for c in cases()]
    return _cache["parsed"]


def pil_flat(p):
    """A parse's coefficients as one image's run of the layout (dummy blocks as PIL coded them: DC of the block before)."""
    return np.concatenate([c.reshape(-1) for c in p["coef"]])


def write_corpus(path, sweep=3):
    """The cases for tests/jpeg_emit_check.cpp: per case int32 {H, W, sampling, quality, sweep?}, int64 n, int16 [n] (PIL's own
    coefficients), int64 size, the file's bytes.  The first `sweep` cases of at most 6 blocks are marked for the capacity sweep."""
    left = sweep
    with open(path, "wb") as f:
        for (name, arr, quality, sampling, blob), p in zip(cases(), parsed()):
            coef = pil_flat(p)
            mark = int(left > 0 and coef.size <= 6 * 64 and arr.shape[0] > 4)
            left -= mark
            f.write(struct.pack("<5iq", arr.shape[0], arr.shape[1], CODE[sampling], quality, mark, coef.size))
            f.write(coef.astype("<i2").tobytes())
            f.write(struct.pack("<q", len(blob)) + blob)
    assert left == 0
