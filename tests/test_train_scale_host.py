"""The premises of tests/test_gpu_train_scale.py, without a GPU: every shape of helpers/train_scale_cases.py takes the branch it was
chosen for -- more work items than one pass of the capped grid (the launch code's formulas restated), a slab plan above the floor
with 900+ slabs and a partial last one, tensors past 2^31 and 2^32 bytes that the entry points' own limits still admit -- and the
tiled method's integer references are the full references' sums, with their exactness premises on the drawn frames and ids."""
import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import first_conv_train_ref as fref
from helpers import fpn_train_ref as pref
from helpers import head_train_ref as href
from helpers import train_scale_cases as cases

f32 = np.float32


# ----------------------------------------------------------------------------- A. the second grid pass
def test_the_grid_caps_are_the_launch_codes():
    """256 * 64 and 256 * 32 blocks of 256 threads (ssd_depthwise_train_backward; conv_train_backward's dilate and ssd_fpn_merge_backward)."""
    assert cases.DW_DX_PASS == 4194304 and cases.MERGE_PASS == cases.DILATE_PASS == 2097152


@pytest.mark.parametrize("case", sorted(cases.A1))
def test_a1_is_just_past_one_pass_of_dw_dx_kernel(case):
    B, H, W, C, stride = cases.A1[case]
    items = cases.dw_dx_items(B, H, W, C)
    assert items == 4194432 and 0 < items - cases.DW_DX_PASS <= 256          # one block of the second pass
    assert B <= 65536 and C % 4 == 0 and C <= 1024 and B * H * W < 2 ** 31
    assert (H ^ W) & 1 == 0 or stride == 1                              # stride 2: one parity, one pad_beg


def test_a1_covers_the_three_instances_of_dw_dx_kernel():
    """<1, 1>, <2, 1> (odd sizes) and <2, 0> (even sizes): (stride, pad_beg of TF 'SAME')."""
    got = {(s, bref.same(H, s)[1]) for _, H, _, _, s in cases.A1.values()}
    assert got == {(1, 1), (2, 1), (2, 0)}


@pytest.mark.parametrize("case", sorted(cases.A2))
def test_a2_is_past_one_pass_of_the_merge_and_its_poison_lies_in_the_second(case):
    B, H, W, C = cases.A2[case]
    rows, quads = B * H * W, (C + 3) // 4
    assert cases.merge_items(B, H, W, C) == rows * quads > cases.MERGE_PASS
    assert rows * quads < 2 * cases.MERGE_PASS                          # and no third pass: the smallest such shape
    first = cases.merge_second_pass_row(C)
    assert (first - 1) * quads < cases.MERGE_PASS <= first * quads and first <= rows - 3
    assert (C % 4 != 0) == (case == "6")                                # 6: the element-wise loads
    assert W % 2 == 1 and C >= 6


def test_a3_is_past_one_pass_of_dilate_permute():
    B, H, W, Cin, Cout = cases.A3
    assert cases.dilate_items(B, H, W, Cout) == 2230272 > cases.DILATE_PASS
    assert Cin % 8 == 0 and B * H * W * max(Cin, Cout, 32) * 4 < 2 ** 31  # conv_plan: every level's tensors below 2 GiB


# ----------------------------------------------------------------------------- B. the slab rule above its floor
def _above_the_floor(plan, R):
    rpp, slab_rows, n_slabs = plan
    return slab_rows > 8 * rpp and n_slabs >= 900 and R % slab_rows != 0


@pytest.mark.parametrize("case", sorted(cases.B1))
def test_b1_plans(case):
    (B, H, W, C, stride), plan = cases.B1[case]
    R = cases.dw_rows(B, H, W, stride)
    assert cases.slab_plan(R, C) == plan and _above_the_floor(plan, R)
    assert plan[0] == 256 // (C // 4)
    assert stride == 1 or (H ^ W) & 1 == 0
    assert R * 9 < 2 ** 24                                              # |x|, |dy| <= 3: the sum of |term| stays an exact float32 integer
    if case == "64-s2":                                                 # just above 1024 slabs of the floor size
        assert 0 < R - 1024 * 8 * plan[0] < 1024


def test_b2_plans():
    for Cout, ((B, H, W, c), plan) in cases.B2.items():
        R = B * (H // 2) * (W // 2)
        assert c == Cout and cases.slab_plan(R, Cout) == plan and R % plan[1] != 0 and plan[2] >= 250
        assert _above_the_floor(plan, R) == (Cout == 32)
        assert B * H * W * 3 < 2 ** 31 and H % 2 == 0 and W % 2 == 0
        assert R * 8 * 2 ** 24 < 2 ** 53                                # |p| <= 2^24 units, |dy| <= 8
    assert cases.B2[24][1][0] == 42 and cases.B2[8][1][1] == 8 * 128


def test_b3_plans():
    for R, C in cases.B3:
        plan = href.slab_plan([R], C)
        assert _above_the_floor(plan, R) and R - 1 >= (plan[2] - 1) * plan[1]
    assert href.slab_plan([8200], 1024) == (1, 9, 912) and 8200 % 9 == 1    # the last slab is the one row that holds the special values
    assert [C for _, C in cases.B3] == [64, 32, 1024]


# ----------------------------------------------------------------------------- C. past 2^31 and 2^32 bytes
@pytest.mark.parametrize("case", sorted(cases.C1))
def test_c1_sizes_limits_and_exactness(case):
    B, H, W, C, stride = cases.C1[case]
    oh, ow = bref.dw_out_hw(H, W, stride)
    frame = H * W * C * 4
    assert B * frame == 4299161600 > 2 ** 32 and B - 2 ** 32 // frame >= 16     # 16 frames wholly above 2^32 bytes
    if stride == 1:
        assert B * oh * ow * C * 4 > 2 ** 32
    # dw_plan's limits
    assert B <= 65536 and H <= 32768 and W <= 32768 and B * H * W < 2 ** 31 and B * H * W * C < 2 ** 40 and C <= 1024 and C % 4 == 0
    assert 2 * B * frame + B * oh * ow * C * 4 <= cases.C1_NEED[case]   # x, dx and dy
    x, _, dy = cases.dw_frames(21 + stride, H, W, C, stride, integers=True)
    ids = cases.ids_of(22 + stride, B)
    assert cases.counts(ids).sum() == B and cases.counts(ids).min() > B // 10
    want, absum = cases.dw_tiled_exact(x, dy, stride, ids)
    assert absum < 2 ** 53 and 0 < np.abs(want).max() < 2 ** 24


def test_c2_sizes_and_limits():
    B, H, W, C = cases.C2
    g_bytes = B * 2 * H * 2 * W * C * 4
    assert g_bytes == 4299161600 > 2 ** 32 and g_bytes // 4 < 2 ** 31 < g_bytes
    assert B <= 65536 and H <= 16384 and W <= 16384 and C <= 4096 and B * H * W * C * 4 < 2 ** 40    # ssd_fpn_merge_backward's refusals
    assert g_bytes + 3 * (g_bytes // 4) <= cases.C2_NEED
    g, base, gate = cases.merge_frames(31, H, W, C)
    want = pref.merge_f32(g, base, gate)
    assert not np.isnan(want).any() and np.isnan(g).sum() == cases.K and np.isnan(gate).sum() == cases.K


def test_c3_sizes_limits_and_exactness():
    B, H, W, Cout = cases.C3
    assert B * H * W * 3 == 415334400 < 2 ** 31                          # fc_plan's limit holds
    dy_bytes = B * (H // 2) * (W // 2) * Cout * 4
    assert dy_bytes == 4430233600 > 2 ** 32 and B * (H // 2) * (W // 2) < 2 ** 31
    assert dy_bytes + B * H * W * 3 <= cases.C3_NEED
    img, dy = cases.fc_data(41, cases.K, H, W, Cout)
    ids = cases.ids_of(42, B)
    units, top = cases.fc_tiled_units(img, dy, ids)
    assert top < 2.0 ** 53 and 0 < np.abs(units).max() < 2 ** 53


# ----------------------------------------------------------------------------- the tiled references are the full references
@pytest.mark.parametrize("stride", [1, 2])
def test_the_tiled_depthwise_sum_is_the_full_batchs(stride):
    H, W, C, B = 5, 7, 8, 23
    x, _, dy = cases.dw_frames(stride, H, W, C, stride, integers=True)
    ids = cases.ids_of(stride + 1, B)
    assert not np.array_equal(ids, np.arange(B) % cases.K)
    want, absum = cases.dw_tiled_exact(x, dy, stride, ids)
    terms = bref.dw_terms(x[ids], dy[ids], stride)
    assert np.array_equal(want.astype(np.float64), terms.sum(0).reshape(3, 3, C, 1)) and absum == np.abs(terms).sum(0).max()
    full, top = cases.dw_exact(x[ids], dy[ids], stride)
    assert np.array_equal(full, want.astype(np.float64)) and top == absum


def test_the_first_convolutions_units_are_fc_terms_and_tile():
    H, W, Cout, B = 6, 8, 8, 17
    img, dy = cases.fc_data(5, cases.K, H, W, Cout)
    units, top = cases.fc_units(img, dy)
    terms = fref.fc_terms(img, dy) * 2.0 ** 24
    assert np.array_equal(units.astype(np.float64), terms.sum(0).reshape(3, 3, 3, Cout)) and top == np.abs(terms).sum(0).max()
    ids = cases.ids_of(6, B)
    tiled, ttop = cases.fc_tiled_units(img, dy, ids)
    terms = fref.fc_terms(img[ids], dy[ids]) * 2.0 ** 24
    assert np.array_equal(tiled.astype(np.float64), terms.sum(0).reshape(3, 3, 3, Cout)) and ttop >= np.abs(terms).sum(0).max()
    assert np.array_equal(cases.units_to_f32(tiled), fref.fc_terms(img[ids], dy[ids]).sum(0).reshape(3, 3, 3, Cout).astype(f32))
