"""The shapes of tests/test_gpu_train_scale.py and the arithmetic that says which branch each one takes: the work items of the three
grid-capped TRAIN kernels against one grid pass (restated from their launch code), the byte sizes of the 4 GiB cases, the entry
points' own limits, and the tiled batches -- K small frames drawn on the CPU and a random assignment ids[b] of one of them to every
frame of the large batch, so that per-image outputs are compared frame by frame with a K-frame call and column sums with
sum_k n_k * T_k in integers.  numpy only: tests/test_train_scale_host.py asserts every premise here without a GPU."""
import numpy as np

from helpers import backbone_train_ref as bref
from helpers import first_conv_train_ref as fref

f32 = np.float32
K = 5                                   # distinct small frames of a tiled batch

# one grid pass of the capped kernels, in work items: blocks * 256 threads (csrc/train_backbone.hip ssd_depthwise_train_backward,
# csrc/train_head.hip conv_train_backward and ssd_fpn_merge_backward)
DW_DX_PASS = 256 * 64 * 256
MERGE_PASS = 256 * 32 * 256
DILATE_PASS = 256 * 32 * 256


# ----------------------------------------------------------------------------- A. a second grid pass
# A1: (B, H, W, C, stride); 3 x 5 at stride 2 has pad_beg 1, 4 x 6 has pad_beg 0: with stride 1 the three instances of dw_dx_kernel
A1 = {"s1": (32769, 3, 5, 128, 1), "s2-pad1": (32769, 3, 5, 128, 2), "s2-pad0": (32769, 4, 6, 128, 2)}
# A2: the OUTPUT's (B, H, W, C); 256: one quad per thread; 6: the element-wise path, two quads per row
A2 = {"256": (2, 128, 129, 256), "6": (2, 512, 1025, 6)}
# A3: (B, H, W, Cin, Cout) of a 3x3 stride-2 convolution
A3 = (2, 66, 66, 8, 256)


def dw_dx_items(B, H, W, C):
    """One thread = 2 rows x 4 pixels x 4 channels of dx."""
    return B * ((H + 1) // 2) * ((W + 3) // 4) * (C // 4)


def merge_items(B, H, W, C):
    """One thread = a channel quad of an output row."""
    return B * H * W * ((C + 3) // 4)


def merge_second_pass_row(C):
    """The first output row whose quads lie in the second grid pass."""
    return -(-MERGE_PASS // ((C + 3) // 4))


def dilate_items(B, H, W, Cout):
    """One thread = an element of the zero-dilated gradient [B,H,W,CinP], CinP = Cout rounded up to 32 (the data gradient's input)."""
    return B * H * W * (-(-Cout // 32) * 32)


# ----------------------------------------------------------------------------- B. the slab rule above its floor
# B1: (B, H, W, C, stride) -> plan (rpp, slab_rows, slabs) of the OUTPUT rows
B1 = {"32": ((5, 230, 230, 32, 1), (32, 288, 919)), "1024": ((2, 65, 64, 1024, 1), (1, 9, 925)),
      "64-s2": ((2, 513, 511, 64, 2), (16, 144, 914))}
# B2: (B, H, W, Cout) -> plan of the B * H/2 * W/2 output rows; 32 leaves the floor, 8 and 24 are many slabs of the floor size
B2 = {32: ((3, 592, 592, 32), (32, 288, 913)), 8: ((3, 592, 592, 8), (128, 1024, 257)), 24: ((3, 592, 592, 24), (42, 336, 783))}
# B3: (rows, C) of one batch-norm level with ReLU6
B3 = [(270000, 64), (264500, 32), (8200, 1024)]


def dw_rows(B, H, W, stride):
    oh, ow = bref.dw_out_hw(H, W, stride)
    return B * oh * ow


# ----------------------------------------------------------------------------- C. offsets past 2^31 and 2^32 bytes
# C1: (B, H, W, C, stride) of a tiled depthwise call | C2: the OUTPUT's (B, H, W, C) of a tiled merge, g [B,2H,2W,C]
# C3: (B, H, W, Cout) of a tiled first-convolution weight gradient
C1 = {"1024": (16400, 8, 8, 1024, 1), "64-s2": (16400, 32, 32, 64, 2)}
C2 = (16400, 8, 8, 256)
C3 = (33800, 64, 64, 32)
GIB = 1 << 30
# device memory a test holds at its peak, in bytes, rounded up to a GiB (the tests' docstrings): C1 x + dy + dx, C2 g + base + gate +
# out, C3 the images + dy -- plus the K frames and the gathered chunks of the comparison
C1_NEED = {"1024": 13 * GIB, "64-s2": 10 * GIB}
C2_NEED = 8 * GIB
C3_NEED = 5 * GIB


# ----------------------------------------------------------------------------- tiled batches
def ids_of(seed, B):
    """A RANDOM assignment of the K small frames to the B frames (b % K would let a wrong batch index through), every one used."""
    ids = np.random.default_rng(seed).integers(0, K, B)
    assert len(np.unique(ids)) == K
    return ids


def counts(ids):
    return np.bincount(ids, minlength=K).astype(np.int64)


def dw_frames(seed, H, W, C, stride, integers):
    """K frames of a depthwise call: x [K,H,W,C], kernel [3,3,C,1], dy [K,OH,OW,C]; integers: x, dy in [-3, 3] (the kernel stays
    random: the weight gradient does not read it)."""
    rng = np.random.default_rng(seed)
    oh, ow = bref.dw_out_hw(H, W, stride)
    k = rng.normal(0, 0.5, (3, 3, C, 1)).astype(f32)
    if integers:
        return rng.integers(-3, 4, (K, H, W, C)).astype(f32), k, rng.integers(-3, 4, (K, oh, ow, C)).astype(f32)
    return rng.normal(0, 1, (K, H, W, C)).astype(f32), k, rng.normal(0, 1, (K, oh, ow, C)).astype(f32)


def dw_tiled_exact(x, dy, stride, ids):
    """The depthwise weight gradient of the tiled batch: sum_k n_k * T_k in int64, T_k frame k's per-tap sums of backbone_train_ref.
    dw_terms.  -> (want int64 [3,3,C,1], the largest sum of |term| over the whole batch)."""
    n = counts(ids)
    want = np.zeros((9, x.shape[3]), np.int64)
    absum = np.zeros((9, x.shape[3]), np.int64)
    for k in range(K):
        t = bref.dw_terms(x[k:k + 1], dy[k:k + 1], stride)
        assert np.array_equal(t, np.round(t))
        want += n[k] * t.sum(0).astype(np.int64)
        absum += n[k] * np.abs(t).sum(0).astype(np.int64)
    return want.reshape(3, 3, -1, 1), int(absum.max())


def dw_exact(x, dy, stride):
    """The depthwise weight gradient of a whole batch on integers, frame by frame through backbone_train_ref.dw_terms (the full
    [rows,9,C] array of the larger cases takes 600 MB).  -> (want float64 [3,3,C,1], the largest sum of |term|)."""
    want = np.zeros((9, x.shape[3]))
    absum = np.zeros((9, x.shape[3]))
    for b in range(x.shape[0]):
        t = bref.dw_terms(x[b:b + 1], dy[b:b + 1], stride)
        want += t.sum(0)
        absum += np.abs(t).sum(0)
    return want.reshape(3, 3, -1, 1), float(absum.max())


def dw_integers(seed, B, H, W, C, stride):
    rng = np.random.default_rng(seed)
    oh, ow = bref.dw_out_hw(H, W, stride)
    return (rng.integers(-3, 4, (B, H, W, C)).astype(f32), rng.integers(-2, 3, (3, 3, C, 1)).astype(f32),
            rng.integers(-3, 4, (B, oh, ow, C)).astype(f32))


def fc_images(rng, B, H, W):
    """Random bytes with 0, 127, 128 and 255 planted on the last row and the last column (tests/test_gpu_first_conv_train.py)."""
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    plant = np.array([0, 127, 128, 255], np.uint8)
    img[:, H - 1, :, :] = plant[rng.integers(0, 4, (B, W, 3))]
    img[:, :, W - 1, :] = plant[rng.integers(0, 4, (B, H, 3))]
    return img


def fc_data(seed, B, H, W, Cout):
    """Frames and an integer dy in [-8, 8] for the first convolution's weight gradient."""
    rng = np.random.default_rng(seed)
    return fc_images(rng, B, H, W), rng.integers(-8, 9, (B, H // 2, W // 2, Cout)).astype(f32)


def fc_units(images, dy):
    """The first convolution's weight gradient in units of 2^-24, exactly: every pixel value is an integer number of units
    (tests/test_first_conv_train_host.py) and dy an integer, so each of the 27 x Cout sums is a sum of integers -- formed here as
    float64 matrix products per tap, which are exact in any order while the sums of magnitudes stay below 2^53 (returned, for the
    caller to assert).  The same numbers as first_conv_train_ref.fc_terms(images, dy).sum(0) * 2^24 without its [R,27,Cout] array
    (1.8 GB at 3 x 592 x 592 x 32).  -> (units int64 [3,3,3,Cout], the largest sum of |term| in units)."""
    B, H, W, _ = images.shape
    OH, OW = H // 2, W // 2
    Cout = dy.shape[3]
    p = fref.pixel_table().astype(np.float64) * 2.0 ** 24
    assert np.array_equal(p, np.round(p))
    x = np.zeros((B, H + 2, W + 2, 3))
    x[:, :H, :W] = p[images]
    d = dy.astype(np.float64).reshape(-1, Cout)
    assert np.array_equal(d, np.round(d))
    units = np.zeros((3, 3, 3, Cout))
    top = 0.0
    for ky in range(3):
        for kx in range(3):
            tap = x[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2].reshape(-1, 3)
            top = max(top, float((np.abs(tap).T @ np.abs(d)).max()))
            units[ky, kx] = tap.T @ d
    assert top < 2.0 ** 53
    return units.astype(np.int64), top


def fc_tiled_units(images, dy, ids):
    """sum_k n_k * T_k of the tiled batch in int64 units of 2^-24.  -> (units [3,3,3,Cout], the largest sum of |term| in units)."""
    n = counts(ids)
    units = np.zeros((3, 3, 3, dy.shape[3]), np.int64)
    top = 0.0
    for k in range(K):
        u, t = fc_units(images[k:k + 1], dy[k:k + 1])
        units += n[k] * u
        top += float(n[k]) * t
    return units, top


def units_to_f32(units):
    """int64 units of 2^-24 below 2^53 in magnitude -> the float32 nearest to the exact sum (one rounding)."""
    assert np.abs(units).max() < 2 ** 53
    return (units.astype(np.float64) * 2.0 ** -24).astype(f32)


def merge_frames(seed, H, W, C):
    """K frames of a merge with same_size = 0: g [K,2H,2W,C], base and gate [K,H,W,C]; every frame's gate starts with -0, 0, NaN, 1,
    -1, Inf and its g has a NaN behind the closed gate at [0,0,0]."""
    rng = np.random.default_rng(seed)
    g, base, gate = (rng.normal(0, 1, s).astype(f32) for s in ((K, 2 * H, 2 * W, C), (K, H, W, C), (K, H, W, C)))
    gate.reshape(K, -1)[:, :6] = [-0.0, 0.0, np.nan, 1.0, -1.0, np.inf]
    g[:, 0, 0, 0] = np.nan
    return g, base, gate


slab_plan = bref.slab_plan                                            # (rows of one level, C) -> (rpp, slab_rows, slabs)
