"""The JPEG decoder's shared case list: small files written at test time with PIL (nothing is committed), and the PIL decode that
every route must reproduce bit for bit -- PIL.Image.open(...).convert("RGB"), the decoder the product used before.

432 files: 12 sizes x {ramp with noise, pure noise} x {4:4:4, 4:2:2, 4:2:0, grayscale} x quality {30, 90, 100} written plainly
(288), and for every (size, sampling, quality) one more with optimised Huffman tables or with restart intervals, in turn (144)."""
import io

import numpy as np

SIZES = [(1, 1), (2, 3), (5, 4), (5, 5), (6, 6), (17, 2), (8, 8), (16, 16), (37, 53), (33, 65), (64, 48), (9, 130)]      # (H, W)
SAMPLINGS = ("444", "422", "420", "gray")
QUALITIES = (30, 90, 100)
_SUB = {"444": 0, "422": 1, "420": 2}


def pixels(h, w, content, seed):
    """uint8 [h, w, 3]: 'ramp' a smooth two-axis ramp per channel with a little noise, 'noise' uniform noise."""
    rng = np.random.default_rng(seed)
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 255.0 * (x + y) / max(h + w - 2, 1)], -1)
    return np.clip(base + rng.normal(0.0, 6.0, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, sampling="420", quality=90, **kw):
    """JPEG bytes of uint8 [H, W, 3] (grayscale: its first channel), written by PIL."""
    from PIL import Image
    im = Image.fromarray(arr[:, :, 0], "L") if sampling == "gray" else Image.fromarray(arr, "RGB")
    buf = io.BytesIO()
    if sampling != "gray":
        kw["subsampling"] = _SUB[sampling]
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pil_rgb(blob):
    """The yardstick: uint8 [H, W, 3]."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


_cache = {}


def cases():
    """[(name, jpeg bytes)] -- built once per process."""
    if "list" not in _cache:
        out, n = [], 0
        for si, (h, w) in enumerate(SIZES):
            for sampling in SAMPLINGS:
                for quality in QUALITIES:
                    for ci, content in enumerate(("ramp", "noise")):
                        arr = pixels(h, w, content, 1000 * si + 10 * quality + ci)
                        out.append(("%dx%d-%s-q%d-%s" % (h, w, sampling, quality, content), encode(arr, sampling, quality)))
                    arr = pixels(h, w, ("ramp", "noise")[n % 2], 7000 + n)
                    if n % 2 == 0:
                        out.append(("%dx%d-%s-q%d-optimize" % (h, w, sampling, quality), encode(arr, sampling, quality, optimize=True)))
                    else:
                        out.append(("%dx%d-%s-q%d-restart%d" % (h, w, sampling, quality, 1 + n % 3),
                                    encode(arr, sampling, quality, restart_marker_blocks=1 + n % 3)))
                    n += 1
        assert len(out) == 432
        _cache["list"] = out
    return _cache["list"]


def expected():
    """[uint8 [H, W, 3]] of cases(), by PIL -- computed once, left unchanged."""
    if "pil" not in _cache:
        _cache["pil"] = [pil_rgb(blob) for _name, blob in cases()]
        for a in _cache["pil"]:
            a.setflags(write=False)
    return _cache["pil"]
