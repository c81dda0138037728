"""The TRAIN step's norms (include/ssd_hip.h, block "the TRAIN step's norms") restated in numpy float64, addition by addition in the
header's order: what csrc/train_norms.hip must match bit for bit.  Independent of the package: nothing is imported from it."""
import numpy as np

BLOCK = 4096                    # SSD_UPDATE_BLOCK_ELEMS
LANES = 256
f64 = np.float64


def squares(x, pad, blocks):
    """x (float32, 1-D) laid out on `blocks` blocks of virtual elements from `pad` -> (float64 squares [blocks * 4096], bad count):
    +0.0 outside the tensor and for a non-finite element.  Adding +0.0 to a sum that started at +0.0 and only grew by squares
    leaves its bits, so "skipped" and "added as +0.0" are the same statement."""
    x = np.asarray(x, np.float32).reshape(-1)
    virt = np.zeros(blocks * BLOCK, f64)
    finite = np.isfinite(x)
    d = np.where(finite, x, np.float32(0)).astype(f64)
    virt[pad:pad + x.size] = d * d                                   # exact: 24 x 24 bits
    bad = np.zeros(blocks * BLOCK, np.int64)
    bad[pad:pad + x.size] = ~finite
    return virt, bad


def block_partials(sq):
    """Stage 1 on the squares of whole blocks [blocks * 4096] -> one float64 partial per block."""
    q = sq.reshape(-1, 4, LANES, 4)                                  # [block, k, lane, e]
    a = np.zeros((q.shape[0], LANES), f64)
    for k in range(4):
        for e in range(4):
            a = a + q[:, k, :, e]                                    # the lane's own elements, in order, from +0.0
    s = LANES // 2
    while s >= 1:
        a = a[:, :s] + a[:, s:2 * s]                                 # a[t] += a[t + s], t < s
        s //= 2
    return a[:, 0]


def ordered_sum(partials):
    """Stage 2: the partials added in ascending order from +0.0."""
    total = f64(0.0)
    for p in partials:
        total = total + f64(p)
    return total


def n_blocks(count, pad):
    return (int(count) + int(pad) + BLOCK - 1) // BLOCK


def tensor_norm(x, pad):
    """(sum of squares, non-finite count) of one array whose first element sits `pad` floats after a 16-byte boundary."""
    x = np.asarray(x, np.float32).reshape(-1)
    blocks = n_blocks(x.size, pad)
    if blocks == 0:
        return f64(0.0), 0
    sq, bad = squares(x, pad, blocks)
    return ordered_sum(block_partials(sq)), int(bad.sum())


def table_norms(tensors):
    """tensors: (w, grad or None, pad of w) per row -> sums float64 [T,2], bad int64 [T,2].  grad's element i goes with w's element
    i: its own alignment never enters."""
    sums = np.zeros((len(tensors), 2), f64)
    bad = np.zeros((len(tensors), 2), np.int64)
    for t, (w, g, pad) in enumerate(tensors):
        sums[t, 0], bad[t, 0] = tensor_norm(w, pad)
        if g is not None:
            assert np.size(g) == np.size(w)
            sums[t, 1], bad[t, 1] = tensor_norm(g, pad)
    return sums, bad
