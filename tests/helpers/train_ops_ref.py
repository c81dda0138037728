"""Float64 numpy restatement of the training convolution (include/ssd_hip.h, "the TRAIN head" and "the TRAIN FPN"): k = 1 or 3 from
the kernel, stride 1 or 2 with conv2d_same's explicit pad, the upsampled operand and the bias, its gradients, and the bounds and
the slice formula that the weight-gradient tests of both blocks use.  The TRAIN head is k = 3, stride 1."""
import numpy as np


def out_hw(H, W, stride):
    return -(-H // stride), -(-W // stride)


def _tap(x, kh, kw, k, stride):
    """x [B,H,W,C] -> what tap (kh,kw) reads per output position: x[b, oy*stride + kh - pad, ox*stride + kw - pad], zero outside."""
    B, H, W, C = x.shape
    pad = (k - 1) // 2
    OH, OW = out_hw(H, W, stride)
    p = np.zeros((B, H + 2 * pad + stride, W + 2 * pad + stride, C), x.dtype)
    p[:, pad:pad + H, pad:pad + W] = x
    return p[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]


def conv(x, w, stride=1, up=None, bias=None):
    k = w.shape[0]
    x, w = x.astype(np.float64), w.astype(np.float64)
    y = 0.0
    for kh in range(k):
        for kw in range(k):
            y = y + _tap(x, kh, kw, k, stride) @ w[kh, kw]
    if up is not None:
        y = y + np.repeat(np.repeat(up.astype(np.float64), 2, axis=1), 2, axis=2)
    return y if bias is None else y + bias.astype(np.float64)


def conv_grads(xs, w, dys, stride=1, absolute=False):
    """Levels xs, dys -> ([dx per level], dw, dbias) in float64; absolute=True: dw = the sums of |x * dy| per element."""
    k = w.shape[0]
    pad = (k - 1) // 2
    w64 = w.astype(np.float64)
    dw = np.zeros(w.shape, np.float64)
    db = np.zeros(w.shape[3], np.float64)
    dxs = []
    for x, dy in zip(xs, dys):
        x, dy = x.astype(np.float64), dy.astype(np.float64)
        B, H, W, C = x.shape
        OH, OW = dy.shape[1:3]
        buf = np.zeros((B, H + 2 * pad + stride, W + 2 * pad + stride, C), np.float64)
        for kh in range(k):
            for kw in range(k):
                a2, d2 = _tap(x, kh, kw, k, stride).reshape(-1, C), dy.reshape(-1, dy.shape[3])
                dw[kh, kw] += np.abs(a2).T @ np.abs(d2) if absolute else a2.T @ d2
                buf[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride] += dy @ w64[kh, kw].T
        dxs.append(buf[:, pad:pad + H, pad:pad + W])
        db += dy.sum((0, 1, 2))
    return dxs, dw, db


def rotated_transposed(w):
    """w'[kh,kw,co,ci] = w[2-kh,2-kw,ci,co]: the data gradient is conv3x3_same(dy, w')."""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def dilate(dy, H, W):
    """D [B,H,W,C]: D[b,2oy,2ox] = dy[b,oy,ox], zero elsewhere (the stride-2 data gradient is conv3x3_same(D, w'))."""
    D = np.zeros((dy.shape[0], H, W, dy.shape[3]), dy.dtype)
    D[:, ::2, ::2] = dy
    return D


def integer_premise(xs, w, dys, stride=1):
    """-> (dw64, dbias64, largest absolute partial sum of dw, of dbias): below 2^24 every partial sum of integers is exact in
    float32 in ANY order."""
    _, dw64, db64 = conv_grads(xs, w, dys, stride)
    _, absum, _ = conv_grads(xs, w, dys, stride, absolute=True)
    return dw64, db64, float(absum.max()), float(sum(np.abs(d).sum((0, 1, 2)).max() for d in dys))


def wgrad_bound(xs, w, dys, stride=1):
    """-> (dw64, bound, absum): |dw - dw64| <= gamma_n * sum|x * dy| per element, n its number of products (output positions whose
    tap lies inside the input), gamma_n = n u / (1 - n u), u = 2^-24: the bound of ANY order of float32 accumulation of exact
    products (the matrix instruction's products are exact in its accumulator's sum)."""
    _, dw64, _ = conv_grads(xs, w, dys, stride)
    _, absum, _ = conv_grads(xs, w, dys, stride, absolute=True)
    _, n, _ = conv_grads([np.ones(x.shape) for x in xs], w, [np.ones(d.shape) for d in dys], stride)
    u = 2.0 ** -24
    return dw64, n * u / (1 - n * u) * absum, absum


def rows_per_slice(out_rows, Cin, Cout, k=3):
    """include/ssd_hip.h's K-slice of the weight gradient for these per-level OUTPUT rows."""
    tiles = k * k * (-(-Cin // 128)) * (-(-Cout // (32 if Cout <= 32 else 128)))
    want = max(1, 1536 // tiles)
    return -(-max(256, -(-sum(out_rows) // want)) // 16) * 16
