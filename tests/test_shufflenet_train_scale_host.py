"""The premises of tests/test_gpu_shufflenet_train_scale.py, without a GPU: every shape of helpers/shufflenet_scale_cases.py takes the
branch it was chosen for -- more work items than one pass of the capped grid (the launch code's formulas restated beside a pointer
to their source), a slab plan above the floor with 900+ slabs and a partial last one, the K-slices of the 1x1 weight gradient,
tensors past 2^31 and 2^32 bytes that the entry points' own limits still admit -- with the exactness premises on the drawn frames,
and the entry points' refusals just outside those limits through the loaded library: they come before any HIP call."""
import ctypes

import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import shufflenet_scale_cases as sc
from helpers import shufflenet_train_ref as ref
from helpers import train_scale_cases as cases

f32 = np.float32


# ----------------------------------------------------------------------------- A. the second grid pass
def test_the_grid_caps_are_the_launch_codes():
    """256 * 64 blocks of 256 threads: launch_depthwise (csrc/elementwise.hip:464, `if (blocks > 256 * 64)`), launch_dw_backward (csrc/
    train_backbone.hip:198, `std::min<long long>((total + 255) / 256, 256 * 64)`) and ssd_sn_maxpool_train_backward (csrc/
    train_shufflenet.hip:256, the same expression); the copies' SN_COPY_MAX_BLOCKS (csrc/train_shufflenet.hip:78) is 256 * 32."""
    assert sc.DW_PASS == sc.POOL_PASS == 4194304 and ref.COPY_MAX_BLOCKS * 256 == 2097152


@pytest.mark.parametrize("case", sorted(sc.A1))
def test_a1_is_just_past_one_pass_of_both_depthwise_kernels(case):
    """Forward (launch_depthwise, csrc/elementwise.hip:461-462): total = B * ceil(OH / R) * ceil(OW / PX) * (C / 2), R, PX = 2, 4 at
    stride 1 and 1, 2 at stride 2.  Data gradient (launch_dw_backward<2>, csrc/train_backbone.hip:197): total = B * ceil(H / 2) *
    ceil(W / 4) * (C / 2).  The second pass holds the last frame and a part of the one before; the drawn assignment gives those two
    frames other small frames than the first two have, and than each other."""
    B, H, W, C, stride = sc.A1[case]
    oh, ow = bref.dw_out_hw(H, W, stride)
    R, PX = (2, 4) if stride == 1 else (1, 2)
    fwd, dx = B * -(-oh // R) * -(-ow // PX) * (C // 2), B * -(-H // 2) * -(-W // 4) * (C // 2)
    assert sc.dw_forward_items(B, H, W, C, stride) == fwd == 4194444 and sc.dw_dx_items(B, H, W, C) == dx == 4194444
    assert fwd - sc.DW_PASS == 140 <= 256                               # one block of the second pass
    assert C % 4 == 2 and sc.lanes(C) == 2 and sc.lanes(8) == 4
    assert B <= 65536 and C <= 1024 and B * H * W < 2 ** 31             # dw_plan's limits
    assert (H ^ W) & 1 == 0 or stride == 1                              # stride 2: one parity, one pad_beg
    per_frame = fwd // B
    assert per_frame == dx // B == 116 and per_frame < 140 <= 2 * per_frame     # the second pass: frames B - 2 (a part) and B - 1
    ids = cases.ids_of(sc.A1_SEEDS[case] + 1, B)
    assert cases.counts(ids).sum() == B and cases.counts(ids).min() > B // 10 and not np.array_equal(ids, np.arange(B) % cases.K)
    assert np.all(ids[-2:] != ids[:2]) and ids[-1] != ids[-2]
    x, _, dy = cases.dw_frames(sc.A1_SEEDS[case], H, W, C, stride, integers=False)
    assert all(not np.array_equal(x[i], x[j]) and not np.array_equal(dy[i], dy[j]) for i in range(cases.K) for j in range(i))


def test_a1_covers_the_five_instances_at_two_channels_per_lane():
    """depthwise_kernel<1, 0, 2, 4, 2> and <2, 0, 1, 2, 2> by stride; dw_dx_kernel<1, 1, 2>, <2, 1, 2> (odd sizes) and <2, 0, 2> (even
    sizes) by (stride, pad_beg of TF 'SAME')."""
    got = {(s, bref.same(H, s)[1]) for _, H, _, _, s in sc.A1.values()}
    assert got == {(1, 1), (2, 1), (2, 0)} and {s for s, _ in got} == {1, 2}


def test_a2_is_just_past_one_pass_of_the_max_pools_gradient():
    """ssd_sn_maxpool_train_backward (csrc/train_shufflenet.hip:255): total = B * H * W * (C / 4)."""
    B, H, W, C = sc.A2
    assert sc.pool_items(B, H, W, C) == B * H * W * (C // 4) == 4194432 and 4194432 - sc.POOL_PASS == 128
    assert H % 2 == 0 and W % 2 == 0 and C % 4 == 0 and B <= 65536
    x, dy = sc.pool_frames(sc.A2_SEED, H, W, C)
    with np.errstate(invalid="ignore"):
        assert (x == 0).sum() > x.size // 4 and np.isnan(x[0, :, :, 1]).all() and np.isnan(x[1, :3, :3, 2]).all()
        assert not np.isnan(x[1, 3:, :, 2]).any()                       # mixed windows beside the all-NaN one
    want = ref.maxpool_grad(x, dy)
    assert not np.isnan(want).any() and np.all(want[0, :, :, 1] == 0) and want[1, 0, 0, 2] == 0 and np.abs(want[1, :, :, 2]).max() > 0
    ids = cases.ids_of(sc.A2_SEED + 1, B)
    assert np.all(ids[-2:] != ids[:2])                                  # 128 items past one pass of 144 per frame: the last frame
    assert cases.counts(ids).sum() == B and cases.counts(ids).min() > B // 10 and not np.array_equal(ids, np.arange(B) % cases.K)


def test_a2_integer_frames_are_tie_free_and_exact():
    _, H, W, C = sc.A2
    xt, dyi = sc.pool_integer_frames(63, H, W, C)
    assert len(np.unique(xt)) == xt.size and np.array_equal(dyi, np.round(dyi))
    _, dxt = ref.torch_maxpool(xt, dyi)
    assert np.array_equal(ref.maxpool_grad(xt, dyi).astype(np.float64), dxt) and np.abs(dxt).max() > 0


@pytest.mark.parametrize("D", [58, 24, 1, 122])
def test_a3_copies_go_past_one_pass(D):
    """launch_sn_copy (csrc/train_shufflenet.hip:127-129): V = 4, 2 or 1 words per access, total = rows * (D / V) threads against
    SN_COPY_MAX_BLOCKS * 256."""
    V = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    rows = ref.copy_rows_past_one_grid_pass(D)
    total, per_pass = rows * (D // V), ref.COPY_MAX_BLOCKS * 256
    assert per_pass < total < 2 * per_pass and total % per_pass
    assert {4 if d % 4 == 0 else 2 if d % 2 == 0 else 1 for d in (58, 24, 1, 122)} == {1, 2, 4}


# ----------------------------------------------------------------------------- B. the slab rule above its floor, K-slices
def _above_the_floor(plan, R):
    rpp, slab_rows, n_slabs = plan
    return slab_rows > 8 * rpp and n_slabs >= 900 and R % slab_rows != 0


def _slab_rule(R, C):
    """include/ssd_hip.h's slab formula, restated (slab_rule, csrc/train_head.h:53): G = ceil(C / 4) channel quads, rpp = 256 / G row
    lanes, slab_rows = max(8 * rpp, ceil(R / 1024)) rounded up to rpp."""
    G = -(-C // 4)
    rpp = 256 // G
    sr = -(-max(8 * rpp, -(-R // 1024)) // rpp) * rpp
    return rpp, sr, -(-R // sr)


@pytest.mark.parametrize("case", sorted(sc.B1))
def test_b1_plans(case):
    (B, H, W, C, stride), plan = sc.B1[case]
    R = cases.dw_rows(B, H, W, stride)
    assert R == {"58": 180000, "58-s2": 180000, "6": 1100000}[case]
    assert sc.slab_plan(R, C) == plan == _slab_rule(R, C) and _above_the_floor(plan, R)
    assert R - (plan[2] - 1) * plan[1] == sc.B1_LAST[case]
    assert C % 4 == 2 and plan[0] == 256 // ((C + 3) // 4)
    if C == 58:                                                         # 15 quads x 17 row lanes = 255 threads: one idle lane per block
        assert plan[0] * ((C + 3) // 4) == 255
    assert stride == 1 or (H ^ W) & 1 == 0
    assert R * 9 < 2 ** 24                                              # |x|, |dy| <= 3: the sum of |term| stays an exact float32 integer
    assert B <= 65536 and C <= 1024 and B * H * W < 2 ** 31


def test_b2_plans():
    for (R, C), plan in sc.B2.items():
        assert sc.bn_plan(R, C) == plan == _slab_rule(R, C) and _above_the_floor(plan, R) and C % 4 == 2
        assert R - (plan[2] - 1) * plan[1] == sc.B2_LAST[(R, C)]
        assert R < 2 ** 26                                              # double_sum_bound's premise
    assert sorted(sc.B2) == [(180000, 58), (180000, 122), (1100000, 6)]


@pytest.mark.parametrize("Cin,Cout", sc.B3_PAIRS)
def test_b3_small_slices(Cin, Cout):
    """conv_plan (csrc/train_head.hip:266-279; wgrad_tile_n, csrc/wgrad.hip:126): tiles = ceil(Cin / 128) * ceil(Cout / BN), BN = 32 for Cout <= 32 and 128 otherwise
    (wgrad_tile_n); rows_per_slice = max(256, ceil(R / (1536 / tiles))) rounded up to 16."""
    B, H, W = sc.B3_SMALL
    R = B * H * W
    assert R == 966
    BN = 32 if Cout <= 32 else 128
    tiles = -(-Cin // 128) * -(-Cout // BN)
    assert tiles == {(130, 58): 2, (58, 130): 2}.get((Cin, Cout), 1)
    rps = -(-max(256, -(-R // (1536 // tiles))) // 16) * 16
    assert sc.slice_plan(R, Cin, Cout) == (rps, -(-R // rps), R - 3 * rps) == (256, 4, 198)
    assert 198 == 12 * 16 + 6                                           # twelve K-steps of WG_BK = 16 rows and 6 rows
    assert Cin % 2 == 0 and Cout % 2 == 0 and (Cin % 4 == 2 or Cout % 4 == 2)      # an 8-byte staging load on one side at least
    if (Cin, Cout) == (130, 58):
        assert Cin - 128 == 2                                           # the second ci tile holds 2 channels
    assert 9 * R < 2 ** 24 and R * sc.pw_widest(Cin, Cout) * 4 < 2 ** 31
    xi, _, dyi = sc.pw_data(Cin * 7 + Cout + 1, B, H, W, Cin, Cout, integers=True)
    want, absum = sc.pw_exact(xi, dyi)
    assert absum <= 9 * R and np.abs(want).max() > 0
    assert np.array_equal(want, np.einsum("bhwi,bhwo->io", xi.astype(np.float64), dyi.astype(np.float64)))


def test_b3_large_slices():
    (B, H, W), (Cin, Cout) = sc.B3_LARGE
    R = B * H * W
    assert R == 400010 and -(-R // 1536) == 261 and -(-261 // 16) * 16 == 272
    assert sc.slice_plan(R, Cin, Cout) == (272, 1471, 170) and 1470 * 272 + 170 == R
    assert sc.pw_widest(Cin, Cout) == 64 and R * 64 * 4 < 2 ** 31 and 9 * R < 2 ** 24


# ----------------------------------------------------------------------------- C. past 2^31 and 2^32 bytes
@pytest.mark.parametrize("case", sorted(sc.C1))
def test_c1_sizes_limits_and_exactness(case):
    B, H, W, C, stride = sc.C1[case]
    oh, ow = bref.dw_out_hw(H, W, stride)
    frame = H * W * C * 4
    assert B * frame == 4418764800 > 2 ** 32 and B - 2 ** 32 // frame >= 16     # 16 frames and more wholly above 2^32 bytes
    assert B * H * W == 19046400 < 2 ** 31
    if stride == 1:
        assert B * oh * ow * C * 4 > 2 ** 32
    # dw_plan's limits
    assert B <= 65536 and H <= 32768 and W <= 32768 and B * H * W * C < 2 ** 40 and C <= 1024 and C % 4 == 2
    assert 2 * B * frame + B * oh * ow * C * 4 <= sc.C1_NEED[case]      # x, dx and dy
    x, _, dy = cases.dw_frames(71 + stride, H, W, C, stride, integers=True)
    ids = cases.ids_of(72 + stride, B)
    assert cases.counts(ids).sum() == B and cases.counts(ids).min() > B // 10
    want, absum = cases.dw_tiled_exact(x, dy, stride, ids)
    assert absum < 2 ** 53 and 0 < np.abs(want).max() < 2 ** 24


def test_c2_sizes_and_limits():
    B, H, W, C = sc.C2
    nbytes = B * H * W * C * 4
    assert nbytes == 4521984000 > 2 ** 32 and B * H * W < 2 ** 31
    assert B <= 65536 and H <= 32768 and W <= 32768 and B * H * W * C < 2 ** 40 and C % 4 == 0 and H % 2 == 0 and W % 2 == 0
    assert 2 * nbytes + nbytes // 4 <= sc.C2_NEED
    assert sc.pool_items(B, H, W, C) > 64 * sc.POOL_PASS
    x, dy = sc.pool_frames(81, H, W, C)
    want = ref.maxpool_grad(x, dy)
    assert not np.isnan(want).any() and np.abs(want).max() > 0


def test_c3_sizes_and_limits():
    rows, D = sc.C3
    assert rows * D * 4 == 4315200000 > 2 ** 32 and 2 * rows * D * 4 > 2 ** 33
    assert D % 4 == 2 and rows < (1 << 40) // D // 2                    # sn_copy_sizes
    assert 6 * rows * D * 4 + 2 * rows * D <= sc.C3_NEED


# ----------------------------------------------------------------------------- refusals just outside the limits
def _aligned(nbytes):
    """A host buffer and a 16-byte aligned address inside it: the calls below never reach a kernel, so no byte of it is read."""
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_depthwise_and_max_pool_refuse_just_outside_their_limits(ssd):
    """dw_plan (csrc/train_backbone.hip:32-33) and ssd_sn_maxpool_train_backward (csrc/train_shufflenet.hip:250-251): B <= 65536, fewer than 2^31 positions and 2^40 elements.
    The largest accepted neighbour gets a positive workspace size (the backward's planner) or passes the size check and is refused
    for its misaligned pointer, still before any HIP call."""
    L = ssd.lib()
    keep, p = _aligned(4096)
    err = lambda: L.ssd_last_error().decode()
    limits = "fewer than 2^31 positions and 2^40 elements"
    fwd = lambda B, H, W, C, x=p: L.ssd_sn_depthwise_train_forward(x, B, H, W, C, p, 1, p, None)
    bwd = lambda B, H, W, C: L.ssd_sn_depthwise_train_backward(p, p, B, H, W, C, p, 1, p, p, p, 1 << 40, None)
    need = lambda B, H, W, C: L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, C, 1)
    pool = lambda B, H, W, C, x=p: L.ssd_sn_maxpool_train_backward(x, p + 1024, B, H, W, C, p + 2048, None)
    outside = [(65537, 2, 2, 58), (32768, 256, 256, 58), (1 << 15, 1 << 7, 1 << 8, 1022 + 4)]
    inside = [(65536, 2, 2, 58), (32768, 256, 254, 58), (1 << 15, 1 << 7, 1 << 8, 1022)]
    assert [B * H * W for B, H, W, _ in outside[1:]] == [2 ** 31, 2 ** 30] and 2 ** 30 * 1026 >= 2 ** 40 > 2 ** 30 * 1022
    # dw_plan checks the positions and the elements before the backward's 1024 channels: 2^30 positions x 1024 channels are 2^40
    # elements and are refused for that by all three calls, as the next even width 1026 is
    for shape in outside + [(1 << 15, 1 << 7, 1 << 8, 1024)]:
        assert fwd(*shape) == -1 and limits in err()
        assert bwd(*shape) == -1 and limits in err()
        assert need(*shape) == 0
    for shape in inside:
        assert need(*shape) > 0
        assert fwd(*shape, x=p + 8) == -1 and "16-byte" in err()
    for shape in [(65537, 2, 2, 24), (32768, 256, 256, 24), (1 << 15, 1 << 7, 1 << 8, 1024)]:
        assert pool(*shape) == -1 and limits in err()
    for shape in [(65536, 2, 2, 24), (32768, 256, 254, 24), (1 << 15, 1 << 7, 1 << 8, 1020)]:
        assert pool(*shape, x=p + 8) == -1 and "16-byte" in err()
    del keep


def test_the_copies_refuse_2_to_the_39_elements(ssd):
    """sn_copy_sizes (csrc/train_shufflenet.hip:141): rows >= 2^40 / D / 2 is refused; the largest accepted rows passes the size check and is refused for its null
    pointer."""
    L = ssd.lib()
    keep, p = _aligned(4096)
    err = lambda: L.ssd_last_error().decode()
    for D in (64, 58):
        edge = (1 << 40) // D // 2
        assert edge * D <= 2 ** 39 < (edge + 1) * D and (D != 64 or edge * D == 2 ** 39)
        for rows, why in ((edge, "2^39"), (edge - 1, "null")):
            assert L.ssd_sn_shuffle_train(p, None, rows, D, 0, p + 1024, p + 2048, None) == -1 and why in err()
            assert L.ssd_sn_shuffle_train(p, None, rows, D, 1, p + 1024, p + 2048, None) == -1 and why in err()
            assert L.ssd_sn_concat_train(p, None, rows, D, p + 1024, None) == -1 and why in err()
            assert L.ssd_sn_split_train(None, rows, D, p + 1024, p + 2048, None) == -1 and why in err()
    del keep


def test_pointwise_refuses_a_level_of_2_gib(ssd):
    """conv_plan (csrc/train_head.hip:253): rows * widest * 4 >= 2^31 is refused, widest = 64 padded channels at 58 -> 58; 2 x 2048 x 2048 rows are exactly 2 GiB,
    2 x 2048 x 2047 rows get a positive workspace size."""
    L = ssd.lib()
    keep, p = _aligned(4096)
    err = lambda: L.ssd_last_error().decode()
    CL = ssd._lib.SsdConvLevel
    lv = lambda H, W: (CL * 1)(CL(H, W, p, p, p))
    assert sc.pw_widest(58, 58) == 64 and 2 * 2048 * 2048 * 64 * 4 == 2 ** 31
    assert L.ssd_sn_pointwise_train_workspace_bytes(lv(2048, 2048), 1, 2, 58, 58) == 0
    assert L.ssd_sn_pointwise_train_forward(lv(2048, 2048), 1, 2, 58, 58, p, p, 1 << 40, None) == -1 and "2 GiB" in err()
    assert L.ssd_sn_pointwise_train_backward(lv(2048, 2048), 1, 2, 58, 58, p, p, p, 1 << 40, None) == -1 and "2 GiB" in err()
    need = L.ssd_sn_pointwise_train_workspace_bytes(lv(2048, 2047), 1, 2, 58, 58)
    assert need > 2 * 2048 * 2047 * 64 * 4
    assert L.ssd_sn_pointwise_train_forward(lv(2048, 2047), 1, 2, 58, 58, p, p, need - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_pointwise_train_backward(lv(2048, 2047), 1, 2, 58, 58, p, p, p, need - 1, None) == -1 and "workspace too small" in err()
    del keep
