"""The JPEG encoder's rules restated in numpy, written from include/ssd_hip.h (block "the JPEG encoder") and not from the kernels:
the quality scaling, the colour conversion, the edge replication, the 2x2 box downsample, the forward DCT and the quantisation as
array arithmetic in int64 (no intermediate leaves int32, so nothing wraps), and the dummy-block rule.

    quant_tables(quality)             -> uint16 [2, 64] (luma, chroma) in natural order
    coefficients(rgb, quality, samp)  -> [int16 [blocks, 64]] * 3 over each component's PADDED grid, the decoder's layout
                                         (tests/helpers/jpeg_ref.parse(...)["coef"])
    flat(coefs)                       -> int16: one image's coefficients as the device stage stores them (dummy blocks ZERO)"""
import numpy as np

LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
SAMPLING = {"444": (1, 1), "420": (2, 2)}


def quant_tables(quality):
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((np.asarray(t, np.int64) * scale + 50) // 100, 1, 255) for t in (LUMA, CHROMA)]).astype(np.uint16)


def ycc(rgb):
    """uint8 [H, W, 3] -> three int64 [H, W] planes."""
    r, g, b = [rgb[:, :, k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _replicate(p, rows, cols):
    """p [m, n] continued to [rows, cols] with its last row and column."""
    yy, xx = np.minimum(np.arange(rows), p.shape[0] - 1), np.minimum(np.arange(cols), p.shape[1] - 1)
    return p[yy][:, xx]


def downsample_h2v2(p, cols):
    """p [H, W] -> [ceil(H / 2), cols]: the columns replicated to 2 * cols BEFORE the box, the rows to an even count; bias 1, 2, 1, .."""
    H = p.shape[0]
    e = _replicate(p, H + (H & 1), 2 * cols)
    bias = 1 + (np.arange(cols) & 1)
    return (e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2] + bias) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """The one-dimensional kernel over the LAST axis; `first`: pass 1's scaling (up by 2 bits), else pass 2's (down by 2 + 13)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0 = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o4 = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o2, o6 = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct_quant(blocks, q):
    """samples int [n, 8, 8], q [64] -> int16 [n, 64]: rows first, then columns, then / (8 q) rounded half away from zero."""
    x = blocks.astype(np.int64) - 128
    rows = _fdct_1d(x, True)                                                 # [n, row, u]
    both = _fdct_1d(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)      # [n, v, u]
    d = 8 * q.astype(np.int64).reshape(1, 8, 8)
    mag = (np.abs(both) + (d >> 1)) // d
    return (np.sign(both) * mag).reshape(-1, 64).astype(np.int16)


def _component(p, own_y, own_x, grid_y, grid_x, q):
    """The plane p (real samples) replicated to its own whole blocks, transformed, and set into the padded grid; every other block
    of the grid is a dummy block: AC zero, DC of the block coded before it (the same component's, in MCU order)."""
    e = _replicate(p, 8 * own_y, 8 * own_x)
    blocks = e.reshape(own_y, 8, own_x, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    real = fdct_quant(blocks, q).reshape(own_y, own_x, 64)
    out = np.zeros((grid_y, grid_x, 64), np.int16)
    out[:own_y, :own_x] = real
    return out


def coefficients(rgb, quality=75, sampling="420", dummy_dc=True):
    h, v = SAMPLING[sampling]
    H, W = rgb.shape[:2]
    q = quant_tables(quality)
    mcus_x, mcus_y = -(-W // (8 * h)), -(-H // (8 * v))
    y, cb, cr = ycc(rgb)
    if (h, v) == (2, 2):
        cb, cr = downsample_h2v2(cb, 8 * mcus_x), downsample_h2v2(cr, 8 * mcus_x)
    luma = _component(y, -(-H // 8), -(-W // 8), mcus_y * v, mcus_x * h, q[0])
    if dummy_dc:
        # MCU order inside the luma grid: the block before (by, bx) is its left neighbour for an odd bx, else (for an odd by) the
        # last block of the row above in the same MCU; dummy blocks chain
        own_y, own_x = -(-H // 8), -(-W // 8)
        for by in range(mcus_y * v):
            for bx in range(mcus_x * h):
                if by >= own_y or bx >= own_x:
                    py, px = (by, bx - 1) if bx % h else (by - 1, bx + h - 1)
                    luma[by, bx, 0] = luma[py, px, 0]
    chroma = [_component(p, mcus_y, mcus_x, mcus_y, mcus_x, q[1]) for p in (cb, cr)]
    return [c.reshape(-1, 64) for c in [luma] + chroma]


def flat(rgb, quality=75, sampling="420"):
    return np.concatenate([c.reshape(-1) for c in coefficients(rgb, quality, sampling, dummy_dc=False)])
