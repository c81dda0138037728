"""The TRAIN step's histograms (include/ssd_hip.h, block "the TRAIN step's histograms") restated in numpy: the limits by the header's
loop, the buckets by np.searchsorted(side="right") on the widened elements, the double sums addition by addition in
helpers/train_norms_ref.py's order: what csrc/train_hist.hip must match bit for bit.  Independent of the package: nothing is
imported from it."""
import sys

import numpy as np

from helpers import train_norms_ref as nref

f32, f64 = np.float32, np.float64
STATS_DTYPE = np.dtype([("sum", "<f8"), ("sum_squares", "<f8"), ("min", "<f4"), ("max", "<f4"), ("num", "<i8"), ("bad", "<i8")])


def limits():
    """The header's loop, one double multiplication per limit."""
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(sys.float_info.max)
    return np.array([-p for p in reversed(pos)] + [0.0] + pos, f64)


LIMITS = limits()
NB = len(LIMITS)


def _ordered(x):
    """float32 values -> uint32 keys whose integer order is the order of the values, -0.0 below +0.0."""
    bits = np.asarray(x, f32).view(np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def plane(x, pad):
    """One plane (float32, 1-D) whose tensor's w sits `pad` floats after a 16-byte boundary -> (counts int64 [NB], stats record)."""
    x = np.asarray(x, f32).reshape(-1)
    finite = np.isfinite(x)
    fx = x[finite]
    counts = np.bincount(np.searchsorted(LIMITS, fx.astype(f64), side="right"), minlength=NB).astype(np.int64)
    assert len(counts) == NB                                         # no finite float reaches DBL_MAX
    st = np.zeros((), STATS_DTYPE)
    st["num"], st["bad"] = int(finite.sum()), int((~finite).sum())
    st["min"], st["max"] = f32(np.inf), f32(-np.inf)
    if len(fx):
        keys = _ordered(fx)
        st["min"], st["max"] = fx[int(np.argmin(keys))], fx[int(np.argmax(keys))]
    blocks = nref.n_blocks(x.size, pad)
    if blocks:
        d = np.where(finite, x, f32(0)).astype(f64)
        virt = np.zeros(blocks * nref.BLOCK, f64)
        virt[pad:pad + x.size] = d
        st["sum"] = nref.ordered_sum(nref.block_partials(virt))
        virt[pad:pad + x.size] = d * d
        st["sum_squares"] = nref.ordered_sum(nref.block_partials(virt))
    return counts, st


def gradient_plane(w, g, decay, weight_decay):
    """The element of plane 1: g + weight_decay * w on a decaying row (one fp32 multiply, one fp32 add), else g."""
    w, g = np.asarray(w, f32).reshape(-1), np.asarray(g, f32).reshape(-1)
    if not decay:
        return g
    with np.errstate(all="ignore"):
        return (g + (f32(weight_decay) * w).astype(f32)).astype(f32)


def table_histograms(tensors, weight_decay):
    """tensors: (w, grad or None, pad of w, decay) per row -> counts int64 [T,2,NB], stats STATS_DTYPE [T,2]."""
    counts = np.zeros((len(tensors), 2, NB), np.int64)
    stats = np.zeros((len(tensors), 2), STATS_DTYPE)
    stats["min"], stats["max"] = f32(np.inf), f32(-np.inf)
    for t, (w, g, pad, decay) in enumerate(tensors):
        counts[t, 0], stats[t, 0] = plane(w, pad)
        if g is not None:
            assert np.size(g) == np.size(w)
            counts[t, 1], stats[t, 1] = plane(gradient_plane(w, g, decay, weight_decay), pad)
    return counts, stats


def compressed(counts):
    """TF's bucket compression of one plane's counts -> (bucket_limit list, bucket list): a run of empty buckets collapses into its
    last bucket with count 0, every non-empty bucket is kept with its limit."""
    lim, bkt = [], []
    i = 0
    while i < NB:
        j = i
        if counts[i] == 0:
            while j + 1 < NB and counts[j + 1] == 0:
                j += 1
        lim.append(float(LIMITS[j]))
        bkt.append(float(counts[j]))
        i = j + 1
    return lim, bkt
