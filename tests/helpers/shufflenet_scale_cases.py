"""The shapes of tests/test_gpu_shufflenet_train_scale.py and the arithmetic that says which branch each one takes: the work items
of the two-channels-per-lane depthwise kernels and of the max pool's gradient against one pass of their capped grids (restated from
the launch code), the slab plans of the weight gradient and the batch norm at C % 4 == 2, the K-slices of the 1x1 weight gradient,
the byte sizes of the 4 GiB cases, the entry points' own limits, and the frames of the tiled batches (helpers/train_scale_cases.py:
K small frames, a random assignment ids[b]).  numpy only: tests/test_shufflenet_train_scale_host.py asserts every premise here
without a GPU."""
import numpy as np

from helpers import backbone_train_ref as bref
from helpers import head_train_ref as href
from helpers.train_scale_cases import GIB, K

f32 = np.float32

# one grid pass of the capped kernels, in work items: 256 * 64 blocks of 256 threads (csrc/elementwise.hip:462-464 launch_depthwise,
# csrc/train_backbone.hip:197-198 launch_dw_backward, csrc/train_shufflenet.hip:255-256 ssd_sn_maxpool_train_backward)
DW_PASS = 256 * 64 * 256
POOL_PASS = 256 * 64 * 256


# ----------------------------------------------------------------------------- A. a second grid pass
# A1: (B, H, W, C, stride) at C % 4 == 2; 3 x 5 at stride 2 has pad_beg 1, 4 x 6 has pad_beg 0: with stride 1 both V = 2 instances of
# depthwise_kernel and all three of dw_dx_kernel
A1 = {"s1": (36159, 3, 5, 58, 1), "s2-pad1": (36159, 3, 5, 58, 2), "s2-pad0": (36159, 4, 6, 58, 2)}
# the seed of A1's K frames; ids come from seed + 1.  The second pass holds the last frame and a part of the one before: the seeds are
# those whose ids[-2:] differ from ids[:2] and from each other, so that a second pass on another frame's data cannot pass (asserted
# in the host file)
A1_SEEDS = {"s1": 55, "s2-pad1": 56, "s2-pad0": 58}
# A2: (B, H, W, C) of the max pool's INPUT; its frames' seed (ids: seed + 1)
A2_SEED = 61
A2 = (29128, 4, 6, 24)


def lanes(C):
    """Channels per lane of the depthwise kernels: 4, or 2 where C % 4 == 2 (launch_depthwise's `pairs`, dw_train_backward's V)."""
    return 4 if C % 4 == 0 else 2


def dw_forward_items(B, H, W, C, stride):
    """launch_depthwise: one thread = R output rows x PX output pixels x V channels, R, PX = 2, 4 at stride 1 and 1, 2 at stride 2."""
    oh, ow = bref.dw_out_hw(H, W, stride)
    R, PX = (2, 4) if stride == 1 else (1, 2)
    return B * (-(-oh // R)) * (-(-ow // PX)) * (C // lanes(C))


def dw_dx_items(B, H, W, C):
    """launch_dw_backward: one thread = 2 rows x 4 pixels x V channels of dx."""
    return B * ((H + 1) // 2) * ((W + 3) // 4) * (C // lanes(C))


def pool_items(B, H, W, C):
    """ssd_sn_maxpool_train_backward: one thread = one input position x 4 channels."""
    return B * H * W * (C // 4)


def pool_frames(seed, H, W, C):
    """K frames of the max pool's gradient: x [K,H,W,C] ReLU-like (about half the taps tie at zero) with one all-NaN channel in frame
    0 and one all-NaN window beside mixed ones in frame 1, dy [K,H/2,W/2,C]."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.normal(0, 1, (K, H, W, C)), 0).astype(f32)
    x[0, :, :, 1] = np.nan
    x[1, :3, :3, 2] = np.nan
    return x, rng.normal(0, 1, (K, H // 2, W // 2, C)).astype(f32)


def pool_integer_frames(seed, H, W, C):
    """K tie-free frames (one permutation of distinct integers over all of them) and an integer dy in [-4, 4]: the gradient's sums
    are exact in any order."""
    rng = np.random.default_rng(seed)
    n = K * H * W * C
    x = (rng.permutation(n).astype(f32) - f32(n // 2)).reshape(K, H, W, C)
    return x, rng.integers(-4, 5, (K, H // 2, W // 2, C)).astype(f32)


# ----------------------------------------------------------------------------- B. the slab rule above its floor, K-slices
# B1: (B, H, W, C, stride) -> plan (rpp, slab_rows, slabs) of the OUTPUT rows; 58: G = 15 quads, rpp = 17 with one idle lane per block
B1 = {"58": ((2, 300, 300, 58, 1), (17, 187, 963)), "58-s2": ((2, 600, 600, 58, 2), (17, 187, 963)),
      "6": ((11, 250, 400, 6, 1), (128, 1152, 955))}
B1_LAST = {"58": 106, "58-s2": 106, "6": 992}                           # rows of the partial last slab
# B2: (rows, C) of one batch-norm level without an activation -> its plan
B2 = {(180000, 58): (17, 187, 963), (180000, 122): (8, 176, 1023), (1100000, 6): (128, 1152, 955)}
B2_LAST = {(180000, 58): 106, (180000, 122): 128, (1100000, 6): 992}
# B3: the 1x1 calls.  Small: (B, H, W) and the (Cin, Cout) pairs; large: one pair
B3_SMALL = (2, 21, 23)
B3_PAIRS = [(58, 58), (24, 58), (58, 24), (122, 122), (130, 58), (58, 130)]
B3_LARGE = ((2, 221, 905), (58, 58))


def slice_plan(R, Cin, Cout):
    """conv_plan's K-slices of a 1x1 weight gradient over R rows of one level (csrc/train_head.hip:266-279, "K-slices of the weight
    gradient"; wgrad_tile_n in csrc/wgrad.hip:126) -> (rows_per_slice, slices, rows of the last slice)."""
    BN = 32 if Cout <= 32 else 128
    tiles = -(-Cin // 128) * -(-Cout // BN)
    want = max(1, 1536 // tiles)
    rps = max(256, -(-R // want))
    rps = -(-rps // 16) * 16
    n = -(-R // rps)
    return rps, n, R - (n - 1) * rps


def pw_widest(Cin, Cout):
    """conv_plan's `widest` (csrc/train_head.hip:244-253): the largest padded channel count of the forward's and the data gradient's
    operands (inputs to a multiple of 32, outputs to a multiple of 8); every level must keep rows * widest * 4 below 2^31."""
    up = lambda v, m: -(-v // m) * m
    return max(up(Cin, 32), up(Cout, 8), up(Cout, 32), up(Cin, 8))


def pw_data(seed, B, H, W, Cin, Cout, integers):
    """x [B,H,W,Cin], the kernel [1,1,Cin,Cout] and dy [B,H,W,Cout]; integers: x, dy in [-3, 3] (the kernel stays random)."""
    rng = np.random.default_rng(seed)
    k = rng.normal(0, 0.1, (1, 1, Cin, Cout)).astype(f32)
    if integers:
        return rng.integers(-3, 4, (B, H, W, Cin)).astype(f32), k, rng.integers(-3, 4, (B, H, W, Cout)).astype(f32)
    return rng.normal(0, 1, (B, H, W, Cin)).astype(f32), k, rng.normal(0, 1, (B, H, W, Cout)).astype(f32)


def pw_exact(x, dy):
    """The 1x1 weight gradient on integers: the float64 matrix product, exact in any order while the sums of magnitudes stay below
    2^53.  -> (want float64 [Cin, Cout], the largest sum of |term|)."""
    a, b = x.reshape(-1, x.shape[-1]).astype(np.float64), dy.reshape(-1, dy.shape[-1]).astype(np.float64)
    assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))
    return a.T @ b, float((np.abs(a).T @ np.abs(b)).max())


# ----------------------------------------------------------------------------- C. offsets past 2^31 and 2^32 bytes
# C1: (B, H, W, C, stride) of a tiled depthwise call | C2: (B, H, W, C) of a tiled max-pool gradient | C3: (rows, D) of the copies
C1 = {"58": (18600, 32, 32, 58, 1), "58-s2": (18600, 32, 32, 58, 2)}
C2 = (46000, 32, 32, 24)
C3 = (18600000, 58)
# device memory a test holds at its peak, in bytes, rounded up to a GiB: C1 x + dy + dx (and, before them, x + out), C2 x + dy + dx
# -- plus the K frames and the gathered chunks of the comparisons --, C3 six tensors of rows * D words (the two inputs, two outputs
# and the restatement of both) and the byte per word of one comparison's mask
C1_NEED = {"58": 13 * GIB, "58-s2": 10 * GIB}
C2_NEED = 10 * GIB
C3_NEED = 27 * GIB

slab_plan = bref.slab_plan                                            # (rows of one level, C) -> (rpp, slab_rows, slabs)
bn_plan = lambda R, C: href.slab_plan([R], C)
