"""include/ssd_hip.h, block "the per-level top losses", restated in numpy: the count rule, the key transform, the k largest keys of
every (plane, image, level) segment in descending order, and the mean over the batch -- the double sum in ascending b from +0.0,
rounded once to float32, then one float32 division.  ssd_loss_top_means is compared with this bit for bit."""
import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32


def counts(anchors_per_level):
    """k_l = ceil(n_l / 5), in integers."""
    return [(int(n) + 4) // 5 for n in anchors_per_level]


def reference_count(n):
    """ssd.py:145 on a level of n anchors: ceil(fp32(n) * fp32(0.20)); n a scalar or an integer array."""
    return np.ceil(np.asarray(n).astype(f32) * f32(0.20)).astype(np.int64)


def keys(x):
    """The uint32 keys whose integer order is the header's total order on float32 bit patterns."""
    bits = np.ascontiguousarray(x, f32).view(u32)
    return bits ^ np.where(bits >> u32(31) != 0, u32(0xFFFFFFFF), u32(0x80000000))


def values(k):
    """The inverse of keys()."""
    k = np.ascontiguousarray(k, u32)
    return (k ^ np.where(k >> u32(31) != 0, u32(0x80000000), u32(0xFFFFFFFF))).view(f32)


def top(segment, k):
    """The k values of a 1-D float32 segment whose keys are largest, in descending key order."""
    return values(np.sort(keys(segment))[::-1][:k])


def selected(planes, anchors_per_level):
    """V: planes float32 [2, B, N] -> float32 [2, B, K], the levels' top values side by side."""
    planes = np.ascontiguousarray(planes, f32)
    assert planes.ndim == 3 and planes.shape[0] == 2 and planes.shape[2] == sum(anchors_per_level)
    ks = counts(anchors_per_level)
    V = np.empty(planes.shape[:2] + (sum(ks),), f32)
    for p in range(2):
        for b in range(planes.shape[1]):
            off = koff = 0
            for n, k in zip(anchors_per_level, ks):
                V[p, b, koff:koff + k] = top(planes[p, b, off:off + n], k)
                off, koff = off + n, koff + k
    return V


def means(planes, anchors_per_level):
    """M float32 [2, K] of planes [2, B, N]."""
    V = selected(planes, anchors_per_level)
    B = V.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((2, V.shape[2]), f64)
        for b in range(B):                                   # ascending b, from +0.0
            s = s + V[:, b].astype(f64)
        return s.astype(f32) / f32(B)


def same_bits(a, b):
    """Bit equality of two float32 arrays, up to NaN payloads that an OPERATION created: the header propagates non-finite values, and
    a sum that creates a NaN (inf - inf) or meets two NaNs does not pin which quiet NaN comes out."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(u32) == b.view(u32)) | both_nan))
