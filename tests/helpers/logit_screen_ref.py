"""Reference side of the class-logit screen (csrc/logit_screen.hip, pack_screen of csrc/weights.hip): numpy, no GPU.

f16_up / f16_down are the directed roundings of the screen's operands.  upper_mark_bound is an upper ENVELOPE of the marks:
whatever a correct screen computes for U on the f16 matrix pipe -- in any summation order, every add off by a relative
2^-22 at most -- stays below U_hi, so a correct screen marks no octet that the envelope leaves unmarked.  Everything here
comes from the operands and the constants of the kernel (2^-9, 2^-18) and of pack_screen (2^-14, 2^-20); nothing from a run."""
import numpy as np

K = 2304                    # 3 x 3 taps x 256 channels: the logits convolution's reduction
U_PIPE = 2.0 ** -22         # the matrix pipe: relative error of one add, at most
E_PIPE = K * U_PIPE         # ... of a sum of K non-negative terms in any order, at most (first order)


def f16_up(v):
    """float64 array >= 0 -> smallest normal f16 value (or inf) >= v; 0 -> 0."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
        low = h.astype(np.float64) < v
        h = np.where(low, np.nextafter(h, np.float16(np.inf)), h)
    out = h.astype(np.float64)
    return np.where(v > 0, np.maximum(out, 2.0 ** -14), 0.0)


def f16_down(v):
    """float64 array >= 0 -> largest normal f16 value <= v (a subnormal result: 0; inf: 65504)."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
        high = h.astype(np.float64) > v
        h = np.where(high, np.nextafter(h, np.float16(-np.inf)), h)
    out = np.minimum(h.astype(np.float64), 65504.0)
    return np.where(out < 2.0 ** -14, 0.0, out)


def patches(tower, level_hw):
    """tower: the oracle's class_tower_3..7, each [B, h, w, 256] (oracle/graph.py, box_predictor) -> the zero-padded 3x3
    patches [rows, 2304], reduction index (ky, kx, channel) as a HWIO kernel flattens, rows in the kernel's order
    (level, image, y, x)."""
    out = []
    for t, (h, w) in zip(tower, level_hw):
        t = np.asarray(t)
        B, c = t.shape[0], t.shape[3]
        assert t.shape[1:3] == (h, w), (t.shape, h, w)
        pad = np.zeros((B, h + 2, w + 2, c), t.dtype)
        pad[:, 1:-1, 1:-1] = t
        taps = [pad[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)]
        out.append(np.stack(taps, axis=3).reshape(B * h * w, 9 * c))
    return np.concatenate(out, axis=0)


def tensor_order(per_row, B, level_hw):
    """[rows, n] in the kernel's row order (level, image, y, x) -> flat, in the order of the logits tensor [B][level, y, x][n]."""
    per_row = np.asarray(per_row)
    parts, r = [], 0
    for h, w in level_hw:
        parts.append(per_row[r:r + B * h * w].reshape(B, -1))
        r += B * h * w
    assert r == per_row.shape[0]
    return np.concatenate(parts, axis=1).reshape(-1)


def screen_constant(wn_sum, bias):
    """cst as pack_screen forms it (float64, rounded up to fp32), then one fp32 ulp higher."""
    b = np.asarray(bias, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        c = b + np.ldexp(np.asarray(wn_sum, np.float64) * (1.0 + 1e-9), -14) + np.ldexp(np.abs(b), -20) + 1e-30
        cst = c.astype(np.float32)
        cst = np.where(cst.astype(np.float64) < c, np.nextafter(cst, np.float32(np.inf)), cst).astype(np.float32)
    return np.nextafter(cst, np.float32(np.inf))


def envelope(P, N, cst):
    """U_hi (fp32) from the exact sums P = sum f16_up(x) f16_up(max(w, 0)), N = sum f16_up(x) f16_down(max(-w, 0)) (float64) and
    cst: the pipe may give P as high as P (1 + e) and N as low as N (1 - e), e = K 2^-22; the result is rounded up to fp32
    and raised by 4 fp32 ulps for the four roundings of the kernel's fp32 epilogue (t1 - t2, + cst, the slack term, the last add)."""
    e = E_PIPE
    c = np.asarray(cst, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        u = (P * (1.0 + e) * (1.0 + 2.0 ** -9) - N * (1.0 - e) * (1.0 - 2.0 ** -9) + c
             + 2.0 ** -18 * (P * (1.0 + e) + N * (1.0 + e) + np.abs(c)))
        f = u.astype(np.float32)
        f = np.where(f.astype(np.float64) < u, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
    for _ in range(4):
        f = np.nextafter(f, np.float32(np.inf))
    return f


def upper_bound(x_patches, kernel, bias, chunk=1024):
    """U_hi [rows, Cout] (fp32) of the logits convolution `kernel` (HWIO [3, 3, 256, Cout]) on the patches [rows, 2304]."""
    w = np.asarray(kernel, np.float64).reshape(-1, np.asarray(kernel).shape[-1])
    nanw = np.isnan(w)
    w = np.where(nanw, 0.0, w)
    wp = f16_up(np.maximum(w, 0.0))
    wn = f16_down(np.maximum(-w, 0.0))
    wp[nanw] = np.nan                       # (pack_screen: a NaN weight goes to Wp)
    cst = screen_constant(wn.sum(axis=0), bias)
    out = np.empty((x_patches.shape[0], w.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(0, x_patches.shape[0], chunk):
            xu = f16_up(np.asarray(x_patches[r:r + chunk], np.float64))
            out[r:r + chunk] = envelope(xu @ wp, xu @ wn, cst[None, :])
    return out


def upper_mark_bound(x_patches, kernel, bias, lo):
    """[rows, Cout / 8] bool: the octets a correct screen MAY mark -- any of its 8 columns has !(U_hi < lo), as the kernel
    writes it (a NaN or an inf marks)."""
    u = upper_bound(x_patches, kernel, bias)
    with np.errstate(invalid="ignore"):
        may = ~(u < np.float32(lo))
    return may.reshape(u.shape[0], -1, 8).any(axis=2)
