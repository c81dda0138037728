"""A numpy float32 restatement of include/ssd_hip.h, block "the TRAIN step's gradient exchange": the bucket layout, one rank's
slice (ssd_train_grad_pack) and the sum of the gathered slices in ascending rank order (ssd_train_grad_reduce).  Written from the
header's text, independently of ssd_amd.train_calls.  numpy's float32 array operations round once each, which is the header's
arithmetic; a NaN that an operation creates (inf - inf), whose sign the header does not pin, is written as CREATED_NAN here, a
value no input of a test holds: `created_nans_as(got, want)` maps whatever NaN the GPU created there to the same value."""
import numpy as np

f32 = np.float32
HEADER_FLOATS = 16
BLOCK = 4096
CREATED_NAN = np.uint32(0x7FC00000)


def created_nans_as(got_bits, want_bits):
    """got_bits (uint32) with every NaN that sits where want_bits holds CREATED_NAN replaced by CREATED_NAN."""
    got_bits = np.array(got_bits, np.uint32)
    there = (np.asarray(want_bits, np.uint32) == CREATED_NAN) & np.isnan(got_bits.view(f32))
    got_bits[there] = CREATED_NAN
    return got_bits


def bucket_layout(counts):
    """(offsets [T], payload floats P, slice floats 16 + P) from the counts alone."""
    offsets, cursor = [], 0
    for n in counts:
        offsets.append(cursor)
        cursor += -(-int(n) // 4) * 4
    P = -(-cursor // BLOCK) * BLOCK
    return offsets, P, HEADER_FLOATS + P


def pack_ref(tensors, counts, header):
    """One rank's slice: tensors[t] a float32 array of counts[t] elements, or None (a NULL row); header 3 floats."""
    offsets, _P, n = bucket_layout(counts)
    out = np.zeros(n, f32)
    out[:3] = np.asarray(header, f32)
    for t, (x, c) in enumerate(zip(tensors, counts)):
        if x is not None:
            out[HEADER_FLOATS + offsets[t]:HEADER_FLOATS + offsets[t] + c] = np.asarray(x, f32).reshape(-1)
    return out


def _at_least_one(a):
    return np.where(a > f32(1), a, f32(1)).astype(f32)


def weights_ref(matches):
    """c_r = max(n_r, 1) / max(S, 1), S added in ascending rank order."""
    n = np.asarray(matches, f32)
    S = n[0]
    for r in range(1, len(n)):
        S = f32(S + n[r])
    return (_at_least_one(n) / _at_least_one(f32(S))).astype(f32)


def _sum(x, c, mean):
    """x [G, ...] -> the header's rule along axis 0."""
    G = x.shape[0]
    with np.errstate(all="ignore"):
        if mean:
            acc = x[0].copy()
            for r in range(1, G):
                acc = acc + x[r]
            acc = acc * (f32(1) / f32(G))
        else:
            acc = x[0] * c[0]
            for r in range(1, G):
                acc = acc + x[r] * c[r]
    acc = np.ascontiguousarray(acc, dtype=f32)
    made = np.isnan(acc) & ~np.isnan(x).any(axis=0)
    acc.view(np.uint32)[made] = CREATED_NAN
    return acc


def reduce_ref(gathered, counts, kinds, present):
    """gathered float32 [G, 16 + P] -> (outs: per row the reduced float32 [count] or None where present[t] is false, losses [2],
    weights [G])."""
    gathered = np.asarray(gathered, f32)
    offsets, _P, n = bucket_layout(counts)
    assert gathered.ndim == 2 and gathered.shape[1] == n
    c = weights_ref(gathered[:, 0])
    losses = _sum(gathered[:, 1:3], c, False)
    outs = []
    for t, cnt in enumerate(counts):
        if not present[t]:
            outs.append(None)
            continue
        lo = HEADER_FLOATS + offsets[t]
        outs.append(_sum(gathered[:, lo:lo + cnt], c, kinds[t] != 0))
    return outs, losses, c
