"""The TRAIN backbone, first convolution and FPN kernels at the sizes where their code takes another path (include/ssd_hip.h, "the
TRAIN backbone", "the TRAIN first convolution", "the TRAIN FPN"): A. the second trip of the grid-stride loop of the three kernels
whose grid is capped (dw_dx_kernel, fpn_merge_backward_kernel, dilate_permute_kernel); B. the slab rule above its floor, about a
thousand slabs with a partial last one, under the depthwise and the first convolution's weight gradients and the batch norm with
ReLU6 at the backbone's widths; C. element offsets past 2^31 and 2^32 bytes in the depthwise forward and backward, the merge's
backward and the first convolution's weight gradient.  Every comparison is exact: bit equality with the CPU oracle or the header's
float32 sequence, exact integers, and the derived bounds of helpers/head_train_ref.py for the batch norm's sums.

The large cases are TILED batches (helpers/train_scale_cases.py): K = 5 small frames are drawn on the CPU, every frame of the large
batch is one of them by a random assignment ids[b], and the large tensors are gathered on the device.  A per-image output must then
have, frame by frame, the bits of a K-frame call that is itself compared with the oracle; a column sum over the batch is
sum_k n_k * T_k in integers.  Outputs are pre-filled with NaN, so a frame that is never written fails.  The shapes and the branch
each one takes are asserted without a GPU in tests/test_train_scale_host.py; measured durations and the free device memory:
profiles/r23_train_scale.log."""
import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import fpn_train_ref as fref
from helpers import head_train_ref as href
from helpers import train_scale_cases as cases
from helpers.backbone_train_gpu import dw_backward_dev, dw_backward_raw, fc_backward_dev, frames_same_bits, same_bits_dev
from helpers.head_train_gpu import bn_raw, conv_backward, conv_backward_raw, dev, same_bits, ulps

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
NAN = float("nan")


def _ids_dev(cuda, ids):
    return cuda.from_numpy(ids).cuda()


# ============================================================================= A. the second grid pass
@pytest.mark.parametrize("case", sorted(cases.A1))
def test_depthwise_data_gradient_past_one_grid_pass(ssd, cuda, oracle_ops, case):
    """dw_dx_kernel's grid is capped at 256 * 64 blocks; 32 769 frames of 3 x 5 (4 x 6) x 128 are 4 194 432 work items, 128 more than
    one pass.  Tiled: the K-frame dx is the oracle's convolution of E bit for bit, every frame of the large dx has the bits of its
    small frame, and the autograd path gives the bits of the raw call (dw included)."""
    B, H, W, C, stride = cases.A1[case]
    assert cases.dw_dx_items(B, H, W, C) > cases.DW_DX_PASS
    x, k, dy = cases.dw_frames(11 + stride + H, H, W, C, stride, integers=False)
    ids = cases.ids_of(12 + stride + H, B)
    sdx, _ = dw_backward_raw(ssd, cuda, x, k, dy, stride)
    want = oracle_ops.depthwise3x3(bref.dilate_E(dy, H, W, stride), bref.flip(k), 1)
    assert sdx.shape == want.shape and np.array_equal(sdx, want) and not np.isnan(sdx).any() and np.abs(sdx).max() > 0
    idv = _ids_dev(cuda, ids)
    X, DY, Kt = dev(cuda, x)[idv], dev(cuda, dy)[idv], dev(cuda, k)
    DX, DW = dw_backward_dev(ssd, cuda, X, Kt, DY, stride)
    bad = frames_same_bits(cuda, DX, dev(cuda, sdx), idv)
    assert bad is None, "dx differs from its small frame in frames %d .. (of %d)" % (bad, B)
    assert bool(cuda.isfinite(DW).all()) and float(DW.abs().max()) > 0
    tx, tk = X.requires_grad_(), Kt.clone().requires_grad_()
    ssd.depthwise_conv(tx, tk, stride).backward(DY)
    assert same_bits_dev(cuda, tx.grad, DX) and same_bits_dev(cuda, tk.grad, DW)


@pytest.mark.parametrize("case", sorted(cases.A2))
def test_merge_backward_past_one_grid_pass(ssd, cuda, case):
    """fpn_merge_backward_kernel's grid is capped at 256 * 32 blocks, one thread per channel quad of an output row.  C = 256: 2 x 128 x
    129 rows are 2 113 536 quads; C = 6 (the element-wise path, two quads per row): 2 x 512 x 1025 rows are 2 099 200.  The gate's
    -0, 0, NaN, 1, -1, Inf and the NaN of g behind a closed gate sit in a row of the SECOND pass.  Both same_size values, with and
    without base and gate, against the header's line bit for bit; out is pre-filled with NaN."""
    B, H, W, C = cases.A2[case]
    rows = B * H * W
    assert cases.merge_items(B, H, W, C) > cases.MERGE_PASS
    row = rows - 3
    assert cases.merge_second_pass_row(C) <= row
    rng = np.random.default_rng(C)
    g, gs, base, gate = (rng.normal(0, 1, s).astype(f32) for s in ((B, 2 * H, 2 * W, C), (B, H, W, C), (B, H, W, C), (B, H, W, C)))
    gate.reshape(rows, C)[row, :6] = [-0.0, 0.0, np.nan, 1.0, -1.0, np.inf]
    b, y, xx = np.unravel_index(row, (B, H, W))
    g[b, 2 * y, 2 * xx, 0] = np.nan                                       # behind the closed gate -0: must not spread
    gs[b, y, xx, 0] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.isnan(gate).any() and (gate > 0).any() and (gate <= 0).any()
    G, GS, BASE, GATE = (dev(cuda, v) for v in (g, gs, base, gate))
    for use_base in (False, True):
        for use_gate in (False, True):
            for same in (False, True):
                out = cuda.full((B, H, W, C), NAN, device="cuda")
                ssd.fpn_merge_backward(GS if same else G, BASE if use_base else None, GATE if use_gate else None, same_size=same, out=out)
                got = out.cpu().numpy()
                want = fref.merge_f32(gs if same else g, base if use_base else None, gate if use_gate else None, same)
                assert same_bits(got, want), (use_base, use_gate, same)
                assert np.isfinite(got.reshape(rows, C)[row, 0]) == use_gate
    tb = dev(cuda, base)                                                # in place: out is base
    ssd.fpn_merge_backward(G, tb, out=tb)
    assert same_bits(tb.cpu().numpy(), fref.merge_f32(g, base))


def test_stride_2_data_gradient_past_one_grid_pass(ssd, cuda, oracle_ops):
    """dilate_permute_kernel's grid is capped at 256 * 32 blocks, one thread per element of the zero-dilated gradient D [B,H,W,CinP]:
    2 x 66 x 66 x 256 = 2 230 272 elements.  dx = conv2d(D, w') of the oracle bit for bit, through the C ABI on a workspace whose
    every byte is 0xFF (a part of D that is never written reads as NaN) and with the same bits through autograd."""
    B, H, W, Cin, Cout = cases.A3
    assert cases.dilate_items(B, H, W, Cout) > cases.DILATE_PASS
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (B, H, W, Cin)).astype(f32)
    dy = rng.normal(0, 1, (B,) + fref.out_hw(H, W, 2) + (Cout,)).astype(f32)
    w = rng.normal(0, 0.05, (3, 3, Cin, Cout)).astype(f32)
    dxs, dw, _ = conv_backward_raw(ssd, cuda, [x], w, [dy], True, False, general=True, stride=2, fill_ws=0xFF)
    want = oracle_ops.conv2d(fref.dilate(dy, H, W), href.rotated_transposed(w))
    assert dxs[0].shape == want.shape and np.array_equal(dxs[0], want) and np.abs(want).max() > 0
    assert np.abs(want[B - 1, H - 1]).max() > 0                           # the last image row, in the second pass, is not all zeros
    ax, aw, _ = conv_backward(ssd, cuda, [x], w, [dy], stride=2, bias=False)
    assert same_bits(ax[0], dxs[0]) and same_bits(aw, dw)


# ============================================================================= B. the slab rule above its floor
def _above_the_floor(plan, R):
    rpp, slab_rows, n_slabs = plan
    return slab_rows > 8 * rpp and n_slabs >= 900 and R % slab_rows != 0


@pytest.mark.parametrize("case", sorted(cases.B1))
def test_depthwise_weight_gradient_over_a_thousand_slabs(ssd, cuda, case):
    """dw_wgrad_partial with slab_rows above its floor 8 * rpp, 900+ slabs into launch_slab_sum and a partial last slab (C = 32: 919
    slabs of 288 rows; C = 1024: 925 of 9; C = 64 at stride 2: 914 of 144): exact on small integers (the premise asserted), two runs
    the same bits."""
    (B, H, W, C, stride), plan = cases.B1[case]
    R = cases.dw_rows(B, H, W, stride)
    assert cases.slab_plan(R, C) == plan and _above_the_floor(plan, R)
    x, k, dy = cases.dw_integers(C + stride, B, H, W, C, stride)
    want, absum = cases.dw_exact(x, dy, stride)
    assert absum < 2 ** 24 and np.abs(want).max() > 0                   # the premise: every partial sum is an exact integer
    X, Kt, DY = dev(cuda, x), dev(cuda, k), dev(cuda, dy)
    _, DW = dw_backward_dev(ssd, cuda, X, Kt, DY, stride, with_dx=False)
    dw = DW.cpu().numpy()
    assert dw.shape == k.shape and np.array_equal(dw.astype(f64), want)
    _, DW2 = dw_backward_dev(ssd, cuda, X, Kt, DY, stride, with_dx=False)
    assert same_bits(dw, DW2.cpu().numpy())


@pytest.mark.parametrize("Cout", sorted(cases.B2))
def test_first_conv_weight_gradient_over_many_slabs(ssd, cuda, Cout):
    """fc_wgrad_partial on 3 frames of 592 x 592, 262 848 output rows.  Cout = 32: slab_rows 288 above the floor 256, 913 slabs; Cout =
    8: 257 slabs of the floor size 1024; Cout = 24: rpp = 42, 783 slabs of 336 -- every last slab partial.  Integer dy in [-8, 8]:
    every term is a multiple of 2^-24 and the sums of magnitudes stay below 2^53 (asserted), so dw is float32(the exact sum)."""
    (B, H, W, _), plan = cases.B2[Cout]
    R = B * (H // 2) * (W // 2)
    assert cases.slab_plan(R, Cout) == plan and plan[2] >= 250 and R % plan[1] != 0
    assert _above_the_floor(plan, R) == (Cout == 32)
    img, dy = cases.fc_data(Cout, B, H, W, Cout)
    units, top = cases.fc_units(img, dy)
    assert top < 2.0 ** 53 and np.abs(units).max() > 0
    want = cases.units_to_f32(units)
    IMG, DY = cuda.from_numpy(img).cuda(), dev(cuda, dy)
    dw = fc_backward_dev(ssd, cuda, IMG, DY).cpu().numpy()
    assert dw.shape == want.shape and same_bits(dw, want)
    assert same_bits(dw, fc_backward_dev(ssd, cuda, IMG, DY).cpu().numpy())


def _same_bits_or_nan(a, b):
    """Bit equality where either is a number; a NaN only has to meet a NaN (its payload is not pinned)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and same_bits(np.where(na, f32(0), a), np.where(nb, f32(0), b))


@pytest.mark.parametrize("R,C", cases.B3)
def test_batch_norm_relu6_over_a_thousand_slabs(ssd, cuda, R, C):
    """ssd_bn_act_train_forward / _backward with ReLU6 on one level of the backbone's widths with slab_rows above its floor (64: 993
    slabs of 272 rows; 32: 919 of 288; 1024: 912 of 9, the last one a single row).  The assertions of tests/test_gpu_backbone_train.py's
    bit-for-bit test: out and dx against the header's float32 sequence on the kernel's own statistics, dgamma / dbeta within the bound
    of a double sum rounded once, two runs the same bits -- and the statistics within one ulp of their float64 definitions.  The
    LAST row, in the partial last slab, holds the y that is exactly 0 (channel 0), the y that is exactly 6 (channel 1: its x makes
    gamma * xhat fall in [4, 8], where 6 - t is exact by Sterbenz) and the NaN (channel 2)."""
    plan = href.slab_plan([R], C)
    assert _above_the_floor(plan, R)
    last = R - 1
    assert last >= (plan[2] - 1) * plan[1]
    rng = np.random.default_rng(C)
    x, dy = rng.normal(0.3, 1.5, (R, C)).astype(f32), rng.normal(0, 1, (R, C)).astype(f32)
    gamma, beta = rng.uniform(2.0, 4.0, C).astype(f32), rng.normal(0, 0.3, C).astype(f32)
    mm, mv = rng.normal(0, 0.1, C).astype(f32), rng.uniform(0.5, 1.5, C).astype(f32)
    x[last, 1] = 0.3 + 2 * 1.5                                           # xhat about 2, gamma in [2, 4]
    x[last, 2] = np.nan
    first = bn_raw(ssd, cuda, [x], [gamma], [beta], [mm], [mv], act="relu6")[0]
    assert same_bits(first["invstd"][[0, 1]], href.invstd_f32(first["var"])[[0, 1]])
    t = ((x[last] - first["mean"]) * (gamma * first["invstd"])).astype(f32)
    beta[0] = -t[0]                                                      # t + (-t) = 0
    assert 3 <= t[1] <= 12
    beta[1] = f32(6) - t[1]
    assert f32(t[1] + beta[1]) == f32(6)
    got = bn_raw(ssd, cuda, [x], [gamma], [beta], [mm], [mv], [dy], act="relu6")[0]
    again = bn_raw(ssd, cuda, [x], [gamma], [beta], [mm], [mv], [dy], act="relu6")[0]
    keep = np.setdiff1d(np.arange(C), [2])
    for name in ("mean", "var", "invstd"):
        assert same_bits(got[name][keep], first[name][keep]) and np.isnan(got[name][2])
    x64 = x[:, keep].astype(f64)
    assert ulps(got["mean"][keep], x64.mean(0).astype(f32)).max() <= 1
    var64 = ((x64 - got["mean"][keep].astype(f64)) ** 2).mean(0)         # the header's variance: around the kernel's own float32 mean
    assert ulps(got["var"][keep], var64.astype(f32)).max() <= 1
    del x64
    ypre, out, dx = bref.bn_act_f32(x, gamma, beta, got["mean"], None, "relu6", dy, dgamma=got["dgamma"], dbeta=got["dbeta"],
                                    invstd=got["invstd"])
    assert ypre[last, 0] == 0 and ypre[last, 1] == 6 and np.isnan(ypre[:, 2]).all()
    opened = bref.gate_f32(ypre, "relu6")
    with np.errstate(invalid="ignore"):
        assert opened.any() and (ypre[:, 3:] <= 0).any() and (ypre[:, 3:] >= 6).any()
    assert same_bits(got["y"], out)
    assert np.all(got["y"][:, 2] == 0) and got["dbeta"][2] == 0            # a NaN y: out 0, gate closed
    assert got["y"][last, 0] == 0 and got["y"][last, 1] == 6 and np.all(got["y"][ypre == 6] == 6) and np.all(got["y"][ypre == 0] == 0)
    assert _same_bits_or_nan(got["dx"], dx)
    gate = np.where(opened, dy, f32(0))[:, keep].astype(f64)
    xhat = ((x - got["mean"]) * got["invstd"]).astype(f32)[:, keep].astype(f64)
    for name, terms in (("dbeta", gate), ("dgamma", gate * xhat)):
        want, tol = href.double_sum_bound(terms)
        err = np.abs(got[name][keep].astype(f64) - want.astype(f64))
        print("batch norm relu6 %d x %d %s: worst |got - exact| / bound = %.3g" % (R, C, name, float((err / tol).max())))
        assert np.all(err <= tol), name
    for name in got:
        assert _same_bits_or_nan(got[name], again[name]), name


# ============================================================================= C. offsets past 2^31 and 2^32 bytes
def _require_free(cuda, need, what):
    """Fails -- it does not skip -- when less than 1.5 x `need` bytes of device memory are free; prints the figure."""
    cuda.cuda.empty_cache()
    free, total = cuda.cuda.mem_get_info()
    print("%s: %.2f GiB of device memory free of %.2f GiB; the test holds %.2f GiB at its peak" % (what, free / cases.GIB, total / cases.GIB, need / cases.GIB))
    if free < 1.5 * need:
        pytest.fail("%s needs %.1f GiB of device memory and asks for 1.5 x that to be free; only %.1f GiB are" % (what, need / cases.GIB, free / cases.GIB))


@pytest.mark.parametrize("case", sorted(cases.C1))
def test_depthwise_forward_and_backward_past_4_gib(ssd, cuda, oracle_ops, case):
    """16 400 tiled frames: 8 x 8 x 1024 at stride 1 (x, out, dy and dx 4 299 161 600 bytes each, 16 frames wholly above 2^32 bytes) and
    32 x 32 x 64 at stride 2 (x and dx that size, out and dy a quarter).  Device memory at the peak (x, dy, dx and the comparison's
    chunks): 13 GiB and 10 GiB.  The forward's out equals ssd.depthwise3x3 of the K frames, gathered; dx equals, frame by frame, the
    K-frame dx that is the oracle's bit for bit; dw is sum_k n_k * T_k exactly (x and dy small integers sharing ids; premises: the
    sum of |term| below 2^53 and |dw| below 2^24)."""
    B, H, W, C, stride = cases.C1[case]
    _require_free(cuda, cases.C1_NEED[case], "depthwise " + case)
    oh, ow = bref.dw_out_hw(H, W, stride)
    x, k, dy = cases.dw_frames(21 + stride, H, W, C, stride, integers=True)
    ids = cases.ids_of(22 + stride, B)
    want_dw, absum = cases.dw_tiled_exact(x, dy, stride, ids)
    assert absum < 2 ** 53 and 0 < np.abs(want_dw).max() < 2 ** 24
    xs, ks, dys, idv = dev(cuda, x), dev(cuda, k), dev(cuda, dy), _ids_dev(cuda, ids)
    sy = ssd.ssd.depthwise3x3(xs, k, stride)
    assert tuple(sy.shape) == (cases.K, oh, ow, C) and not bool(cuda.isnan(sy).any()) and float(sy.abs().max()) > 0
    sdx, _ = dw_backward_dev(ssd, cuda, xs, ks, dys, stride)
    want = oracle_ops.depthwise3x3(bref.dilate_E(dy, H, W, stride), bref.flip(k), 1)
    assert np.array_equal(sdx.cpu().numpy(), want) and not np.isnan(want).any() and np.abs(want).max() > 0
    X = xs[idv]
    assert X.numel() * 4 > 2 ** 32
    OUT = cuda.full((B, oh, ow, C), NAN, device="cuda")
    ssd.train_calls.depthwise_forward(X, ks, OUT, stride)
    bad = frames_same_bits(cuda, OUT, sy, idv)
    assert bad is None, "out differs from its small frame in frames %d .. (of %d)" % (bad, B)
    del OUT
    DY = dys[idv]
    DX, DW = dw_backward_dev(ssd, cuda, X, ks, DY, stride)
    bad = frames_same_bits(cuda, DX, sdx, idv)
    assert bad is None, "dx differs from its small frame in frames %d .. (of %d)" % (bad, B)
    assert np.array_equal(DW.cpu().numpy().astype(f64), want_dw.astype(f64))


def test_merge_backward_past_4_gib(ssd, cuda):
    """same_size = 0 on 16 400 tiled frames: g [B,16,16,256] is 4 299 161 600 bytes, base, gate and out [B,8,8,256] a quarter each; 8 GiB
    of device memory at the peak.  Every frame's gate holds -0, 0, NaN, 1, -1, Inf and its g a NaN behind a closed gate.  The K-frame
    out is the header's line bit for bit and has no NaN; every frame of the large out has the bits of its small frame."""
    B, H, W, C = cases.C2
    _require_free(cuda, cases.C2_NEED, "merge")
    g, base, gate = cases.merge_frames(31, H, W, C)
    ids = cases.ids_of(32, B)
    gs, bs, gts, idv = dev(cuda, g), dev(cuda, base), dev(cuda, gate), _ids_dev(cuda, ids)
    small = cuda.full((cases.K, H, W, C), NAN, device="cuda")
    ssd.fpn_merge_backward(gs, bs, gts, out=small)
    want = fref.merge_f32(g, base, gate)
    assert same_bits(small.cpu().numpy(), want) and not np.isnan(want).any() and np.abs(want).max() > 0
    G, BASE, GATE = gs[idv], bs[idv], gts[idv]
    assert G.numel() * 4 > 2 ** 32
    OUT = cuda.full((B, H, W, C), NAN, device="cuda")
    ssd.fpn_merge_backward(G, BASE, GATE, out=OUT)
    bad = frames_same_bits(cuda, OUT, small, idv)
    assert bad is None, "out differs from its small frame in frames %d .. (of %d)" % (bad, B)


def test_first_conv_weight_gradient_past_4_gib(ssd, cuda):
    """33 800 tiled frames of 64 x 64: the images are 415 334 400 bytes (B * H * W * 3 below 2^31, the entry point's limit), dy [B,32,32,32]
    is 4 430 233 600 bytes; 5 GiB of device memory at the peak.  Integer dy: dw is float32(sum_k n_k * T_k), T_k in units of 2^-24,
    the sums of magnitudes below 2^53 (asserted)."""
    B, H, W, Cout = cases.C3
    _require_free(cuda, cases.C3_NEED, "first convolution")
    img, dy = cases.fc_data(41, cases.K, H, W, Cout)
    ids = cases.ids_of(42, B)
    units, top = cases.fc_tiled_units(img, dy, ids)
    assert top < 2.0 ** 53 and np.abs(units).max() > 0
    imgs, dys, idv = cuda.from_numpy(img).cuda(), dev(cuda, dy), _ids_dev(cuda, ids)
    small = fc_backward_dev(ssd, cuda, imgs, dys).cpu().numpy()
    assert same_bits(small, cases.units_to_f32(cases.fc_units(img, dy)[0]))
    IMG, DY = imgs[idv], dys[idv]
    assert IMG.numel() < 2 ** 31 and DY.numel() * 4 > 2 ** 32
    dw = fc_backward_dev(ssd, cuda, IMG, DY).cpu().numpy()
    assert same_bits(dw, cases.units_to_f32(units))
