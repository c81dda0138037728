"""The TRAIN ShuffleNet's kernels at the sizes where their code takes another path (include/ssd_hip.h, "the TRAIN ShuffleNet"): A. the
second trip of the grid-stride loop of the two-channels-per-lane depthwise kernels (C = 58: depthwise_kernel<.., V = 2> and
dw_dx_kernel<.., 2>) and of maxpool_backward_kernel; B. the slab rule above its floor, about a thousand slabs with a partial last
one, under dw_wgrad_partial<2> and the batch norm without an activation at C % 4 == 2, and the 1x1 weight gradient in more than
one K-slice at even widths; C. element offsets past 2^31 and 2^32 bytes in the depthwise forward and backward at C = 58, the max
pool's gradient and the four copies.  Every comparison is exact: bit equality with the CPU oracle or the header's float32 sequence,
exact integers, and the derived bound of helpers/head_train_ref.py for the batch norm's double sums.

The large per-image cases are TILED batches (helpers/train_scale_cases.py): K = 5 small frames drawn on the CPU, a random assignment
ids[b], the large tensors gathered on the device; every frame of a large output must have the bits of its small frame, whose K-frame
call is itself compared with the oracle.  Outputs are pre-filled with NaN, so a frame that is never written fails.  The shapes and
the branch each one takes are asserted without a GPU in tests/test_shufflenet_train_scale_host.py; measured durations and the free
device memory: profiles/r27_shufflenet_train_scale.log."""
import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import head_train_ref as href
from helpers import shufflenet_scale_cases as sc
from helpers import shufflenet_train_ref as ref
from helpers import train_scale_cases as cases
from helpers.backbone_train_gpu import dw_backward_dev, dw_backward_raw, frames_same_bits, same_bits_dev
from helpers.head_train_gpu import dev, same_bits
from helpers.shufflenet_train_gpu import bn_raw, dw_forward, pw

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
NAN = float("nan")
SN = "sn_depthwise"


def _ids_dev(cuda, ids):
    return cuda.from_numpy(ids).cuda()


def _bits(cuda, a):
    """Any bit pattern of a float32 numpy array on the device (no conversion touches a NaN's payload)."""
    return cuda.from_numpy(np.ascontiguousarray(a, dtype=f32).view(np.int32).copy()).cuda().view(cuda.float32)


def _tiled_depthwise(ssd, cuda, oracle_ops, B, H, W, C, stride, seed):
    """The K-frame forward and data gradient at C % 4 == 2 against the oracle bit for bit, then the tiled batch of B frames: out and
    dx frame by frame against the K-frame calls.  -> (X, Kt, DY, OUT, DX, DW) on the device."""
    x, k, dy = cases.dw_frames(seed, H, W, C, stride, integers=False)
    ids = cases.ids_of(seed + 1, B)
    sy = dw_forward(ssd, cuda, x, k, stride, SN)
    assert same_bits(sy, oracle_ops.depthwise3x3(x, k, stride)) and not np.isnan(sy).any() and np.abs(sy).max() > 0
    sdx, _ = dw_backward_raw(ssd, cuda, x, k, dy, stride, entry=SN)
    want = oracle_ops.depthwise3x3(bref.dilate_E(dy, H, W, stride), bref.flip(k), 1)
    assert sdx.shape == want.shape and same_bits(sdx, want) and not np.isnan(sdx).any() and np.abs(sdx).max() > 0
    idv = _ids_dev(cuda, ids)
    X, DY, Kt = dev(cuda, x)[idv], dev(cuda, dy)[idv], dev(cuda, k)
    OUT = cuda.full(tuple(DY.shape), NAN, device="cuda")
    ssd.train_calls.depthwise_forward(X, Kt, OUT, stride, entry=SN)
    bad = frames_same_bits(cuda, OUT, dev(cuda, sy), idv)
    assert bad is None, "out differs from its small frame in frames %d .. (of %d)" % (bad, B)
    DX, DW = dw_backward_dev(ssd, cuda, X, Kt, DY, stride, entry=SN)
    bad = frames_same_bits(cuda, DX, dev(cuda, sdx), idv)
    assert bad is None, "dx differs from its small frame in frames %d .. (of %d)" % (bad, B)
    return X, Kt, DY, OUT, DX, DW


# ============================================================================= A. the second grid pass
@pytest.mark.parametrize("case", sorted(sc.A1))
def test_depthwise_at_58_channels_past_one_grid_pass(ssd, cuda, oracle_ops, case):
    """depthwise_kernel<.., V = 2> and dw_dx_kernel<S, P, 2>: both grids are capped at 256 * 64 blocks; 36 159 frames of 3 x 5 (4 x 6) x
    58 are 4 194 444 work items of 2 channels in the forward and in the data gradient, 140 more than one pass.  Tiled: the K-frame
    calls are the oracle's bit for bit, every frame of the large out and dx has the bits of its small frame, dw is finite and not
    zero, and the autograd path gives the bits of the raw calls (dw included)."""
    B, H, W, C, stride = sc.A1[case]
    assert sc.dw_forward_items(B, H, W, C, stride) > sc.DW_PASS and sc.dw_dx_items(B, H, W, C) > sc.DW_PASS and C % 4 == 2
    X, Kt, DY, OUT, DX, DW = _tiled_depthwise(ssd, cuda, oracle_ops, B, H, W, C, stride, sc.A1_SEEDS[case])
    assert bool(cuda.isfinite(DW).all()) and float(DW.abs().max()) > 0
    tx, tk = X.requires_grad_(), Kt.clone().requires_grad_()
    ty = ssd.depthwise_conv(tx, tk, stride)
    ty.backward(DY)
    assert same_bits_dev(cuda, ty.detach(), OUT) and same_bits_dev(cuda, tx.grad, DX) and same_bits_dev(cuda, tk.grad, DW)


def _pool_grad_dev(ssd, cuda, X, DY):
    DX = cuda.full_like(X, NAN)
    ssd.train_calls.maxpool_backward(X, DY, DX)
    return DX


def _tiled_pool(ssd, cuda, B, H, W, C, seed):
    """The K-frame gradient of the max pool against the restated tie rule bit for bit, then every frame of the tiled batch."""
    x, dy = sc.pool_frames(seed, H, W, C)
    assert (x == 0).sum() > x.size // 4 and np.isnan(x[0, :, :, 1]).all() and np.isnan(x[1, :3, :3, 2]).all()
    xs, dys = _bits(cuda, x), dev(cuda, dy)
    small = _pool_grad_dev(ssd, cuda, xs, dys)
    want = ref.maxpool_grad(x, dy)
    got = small.cpu().numpy()
    assert same_bits(got, want) and not np.isnan(want).any() and np.abs(want).max() > 0
    assert np.all(got[0, :, :, 1] == 0) and got[1, 0, 0, 2] == 0       # no winner in an all-NaN window
    idv = _ids_dev(cuda, cases.ids_of(seed + 1, B))
    X, DY = xs[idv], dys[idv]
    DX = _pool_grad_dev(ssd, cuda, X, DY)
    bad = frames_same_bits(cuda, DX, small, idv)
    assert bad is None, "dx differs from its small frame in frames %d .. (of %d)" % (bad, B)
    return X, idv


def test_max_pool_gradient_past_one_grid_pass(ssd, cuda):
    """maxpool_backward_kernel's grid is capped at 256 * 64 blocks, one thread per input position and channel quad: 29 128 frames of
    4 x 6 x 24 are 4 194 432 work items, 128 more than one pass.  Tiled: ReLU-like frames (about half the taps tie at zero), an
    all-NaN channel in one frame and an all-NaN window beside mixed ones in another; the K-frame dx is the restated tie rule's bit for
    bit, every frame of the large dx has the bits of its small frame.  On tie-free integer frames the K-frame dx is torch
    autograd's exactly, and ssd.maxpool3x3s2_train through autograd gives the raw call's values on the large batch."""
    B, H, W, C = sc.A2
    assert sc.pool_items(B, H, W, C) > sc.POOL_PASS
    _, idv = _tiled_pool(ssd, cuda, B, H, W, C, sc.A2_SEED)
    xt, dyi = sc.pool_integer_frames(63, H, W, C)
    _, dxt = ref.torch_maxpool(xt, dyi)
    xts, dyis = dev(cuda, xt), dev(cuda, dyi)
    assert np.array_equal(_pool_grad_dev(ssd, cuda, xts, dyis).cpu().numpy().astype(f64), dxt) and np.abs(dxt).max() > 0
    XT, DYI = xts[idv], dyis[idv]
    raw = _pool_grad_dev(ssd, cuda, XT, DYI)
    tx = XT.clone().requires_grad_()
    ssd.maxpool3x3s2_train(tx).backward(DYI)
    assert same_bits_dev(cuda, tx.grad, raw) and frames_same_bits(cuda, raw, dev(cuda, dxt.astype(f32)), idv) is None


# ============================================================================= B. the slab rule above its floor, K-slices
def _above_the_floor(plan, R):
    rpp, slab_rows, n_slabs = plan
    return slab_rows > 8 * rpp and n_slabs >= 900 and R % slab_rows != 0


@pytest.mark.parametrize("case", sorted(sc.B1))
def test_depthwise_weight_gradient_at_even_widths_over_a_thousand_slabs(ssd, cuda, case):
    """dw_wgrad_partial<2> with slab_rows above its floor 8 * rpp, 900+ slabs into launch_slab_sum and a partial last slab (C = 58 at
    either stride: G = 15 quads of which the last is half outside, rpp = 17 with one idle lane per block, 963 slabs of 187 rows, the
    last of 106; C = 6: 955 slabs of 1152 rows, the last of 992): exact on small integers (the premise asserted), two runs the same
    bits."""
    (B, H, W, C, stride), plan = sc.B1[case]
    R = cases.dw_rows(B, H, W, stride)
    assert sc.slab_plan(R, C) == plan and _above_the_floor(plan, R) and C % 4 == 2
    x, k, dy = cases.dw_integers(C + stride, B, H, W, C, stride)
    want, absum = cases.dw_exact(x, dy, stride)
    assert absum < 2 ** 24 and np.abs(want).max() > 0                   # the premise: every partial sum is an exact integer
    X, Kt, DY = dev(cuda, x), dev(cuda, k), dev(cuda, dy)
    _, DW = dw_backward_dev(ssd, cuda, X, Kt, DY, stride, with_dx=False, entry=SN)
    dw = DW.cpu().numpy()
    assert dw.shape == k.shape and np.array_equal(dw.astype(f64), want)
    _, DW2 = dw_backward_dev(ssd, cuda, X, Kt, DY, stride, with_dx=False, entry=SN)
    assert same_bits(dw, DW2.cpu().numpy())


@pytest.mark.parametrize("R,C", sorted(sc.B2))
def test_batch_norm_without_activation_over_a_thousand_slabs(ssd, cuda, R, C):
    """ssd_sn_bn_train_forward / _backward with SSD_ACT_NONE at C % 4 == 2 with slab_rows above its floor (58: 963 slabs of 187 rows;
    122: 1023 of 176; 6: 955 of 1152 -- every last slab partial).  The assertions of tests/test_gpu_shufflenet_train.py's bit-for-bit
    test: the statistics have the bits of the ReLU call's, invstd and the moving update are the header's, y and dx are the header's
    float32 sequence on the kernel's own statistics bit for bit, dgamma and dbeta lie within the bound of a double sum rounded once
    (the worst fraction of it is printed), two calls give the same bits."""
    plan = sc.bn_plan(R, C)
    assert plan == sc.B2[(R, C)] and _above_the_floor(plan, R) and C % 4 == 2
    rng = np.random.default_rng(C)
    x, dy = rng.normal(0.3, 1.5, (R, C)).astype(f32), rng.normal(0, 1, (R, C)).astype(f32)
    gamma, beta = rng.uniform(2.0, 4.0, C).astype(f32), rng.normal(0, 0.3, C).astype(f32)
    mm, mv = rng.normal(0, 0.1, C).astype(f32), rng.uniform(0.5, 1.5, C).astype(f32)
    g = bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy)
    relu = bn_raw(ssd, cuda, x, gamma, beta, mm, mv, act="relu", entry="bn_act")
    for name in ("mean", "var", "invstd", "mm", "mv"):
        assert same_bits(g[name], relu[name]), name
    assert same_bits(g["invstd"], href.invstd_f32(g["var"])) and np.all(np.abs(g["mean"] - x.mean(0, dtype=f64)) < 1e-5)
    wm, wv = href.moving_update(mm, mv, g["mean"], g["var"], R)
    assert same_bits(g["mm"], wm) and same_bits(g["mv"], wv) and not same_bits(g["mm"], mm)
    y, dx = ref.bn_none_f32(x, gamma, beta, g["mean"], g["invstd"], dy, g["dgamma"], g["dbeta"])
    assert same_bits(g["y"], y) and (y < 0).any() and (y > 6).any()                     # nothing is clipped
    assert same_bits(g["dx"], dx) and np.abs(dx).max() > 0
    xhat = ((x - g["mean"]) * g["invstd"]).astype(f32).astype(f64)
    for name, terms in (("dbeta", dy.astype(f64)), ("dgamma", dy.astype(f64) * xhat)):  # g = dy: every gate is open
        want, tol = href.double_sum_bound(terms)
        err = np.abs(g[name].astype(f64) - want.astype(f64))
        print("batch norm none %d x %d %s: worst |got - exact| / bound = %.3g" % (R, C, name, float((err / tol).max())))
        assert np.all(err <= tol), name
    again = bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy)
    for name in g:
        assert same_bits(g[name], again[name]), name


def _pointwise(ssd, cuda, oracle_ops, B, H, W, Cin, Cout):
    """The assertions of tests/test_gpu_shufflenet_train.py's 1x1 test on one level of B x H x W rows, and two runs the same bits."""
    R = B * H * W
    x, k, dy = sc.pw_data(Cin * 7 + Cout, B, H, W, Cin, Cout, integers=False)
    y, dx, dw = pw(ssd, cuda, x, k, dy, "sn_pointwise")
    assert same_bits(y, ssd.ssd.conv2d(dev(cuda, x), k).cpu().numpy()) and not np.isnan(y).any() and np.abs(y).max() > 0
    want = oracle_ops.conv2d(dy, np.ascontiguousarray(k.transpose(0, 1, 3, 2)))
    assert dx.shape == want.shape and same_bits(dx, want) and np.abs(dx).max() > 0
    assert np.isfinite(dw).all() and np.abs(dw).max() > 0
    tx, tk = dev(cuda, x).requires_grad_(), dev(cuda, k).requires_grad_()
    ty = ssd.pointwise_conv(tx, tk)
    ty.backward(dev(cuda, dy))
    assert same_bits(ty.detach().cpu().numpy(), y) and same_bits(tx.grad.cpu().numpy(), dx) and same_bits(tk.grad.cpu().numpy(), dw)
    for a, b in zip((y, dx, dw), pw(ssd, cuda, x, k, dy, "sn_pointwise")):
        assert same_bits(a, b)
    xi, _, dyi = sc.pw_data(Cin * 7 + Cout + 1, B, H, W, Cin, Cout, integers=True)
    wanti, absum = sc.pw_exact(xi, dyi)
    assert 9 * R < 2 ** 24 and absum < 2 ** 24 and np.abs(wanti).max() > 0   # the premise: every partial sum is an exact integer
    _, _, dwi = pw(ssd, cuda, xi, k, dyi, "sn_pointwise")
    assert dwi.shape == k.shape and np.array_equal(dwi.reshape(Cin, Cout).astype(f64), wanti)
    _, _, dwi2 = pw(ssd, cuda, xi, k, dyi, "sn_pointwise")
    assert same_bits(dwi, dwi2)


@pytest.mark.parametrize("Cin,Cout", sc.B3_PAIRS)
def test_pointwise_weight_gradient_in_four_slices_at_even_widths(ssd, cuda, oracle_ops, Cin, Cout):
    """wgrad_kernel with th_width(Cin) or th_width(Cout) equal to 2 on 2 x 21 x 23 = 966 rows: four K-slices of 256 rows, the last of
    198 (twelve K-steps and 6 rows).  (130, 58) has two ci tiles, the second with 2 channels; (58, 130) has two co tiles.  Forward =
    ssd.conv2d and dx = the oracle's conv2d(dy, w') bit for bit, dw exact on integers |v| <= 3, autograd the raw call's bits."""
    B, H, W = sc.B3_SMALL
    assert sc.slice_plan(B * H * W, Cin, Cout) == (256, 4, 198)
    _pointwise(ssd, cuda, oracle_ops, B, H, W, Cin, Cout)


def test_pointwise_weight_gradient_in_1471_slices_at_58_channels(ssd, cuda, oracle_ops):
    """2 x 221 x 905 = 400 010 rows, 58 -> 58: 1471 K-slices of 272 rows, the last of 170, added by wgrad_reduce in ascending order."""
    (B, H, W), (Cin, Cout) = sc.B3_LARGE
    assert sc.slice_plan(B * H * W, Cin, Cout) == (272, 1471, 170)
    _pointwise(ssd, cuda, oracle_ops, B, H, W, Cin, Cout)


# ============================================================================= C. offsets past 2^31 and 2^32 bytes
def _require_free(cuda, need, what):
    """Fails -- it does not skip -- when less than 1.5 x `need` bytes of device memory are free; prints the figure."""
    cuda.cuda.empty_cache()
    free, total = cuda.cuda.mem_get_info()
    print("%s: %.2f GiB of device memory free of %.2f GiB; the test holds %.2f GiB at its peak" % (what, free / cases.GIB, total / cases.GIB, need / cases.GIB))
    if free < 1.5 * need:
        pytest.fail("%s needs %.1f GiB of device memory and asks for 1.5 x that to be free; only %.1f GiB are" % (what, need / cases.GIB, free / cases.GIB))


@pytest.mark.parametrize("case", sorted(sc.C1))
def test_depthwise_at_58_channels_past_4_gib(ssd, cuda, oracle_ops, case):
    """18 600 tiled frames of 32 x 32 x 58 at stride 1 (x, out, dy and dx 4 418 764 800 bytes each) and at stride 2 (x and dx that size,
    out and dy a quarter); 19.0 M positions.  Device memory at the peak (x, dy, dx and the comparison's chunks): 13 GiB and 10 GiB.
    The K-frame out and dx are the oracle's bit for bit, every frame of the large out and dx has the bits of its small frame; dw is
    sum_k n_k * T_k exactly (x and dy small integers sharing ids; premises: the sum of |term| below 2^53 and |dw| below 2^24)."""
    B, H, W, C, stride = sc.C1[case]
    _require_free(cuda, sc.C1_NEED[case], "depthwise " + case)
    oh, ow = bref.dw_out_hw(H, W, stride)
    x, k, dy = cases.dw_frames(71 + stride, H, W, C, stride, integers=True)
    ids = cases.ids_of(72 + stride, B)
    want_dw, absum = cases.dw_tiled_exact(x, dy, stride, ids)
    assert absum < 2 ** 53 and 0 < np.abs(want_dw).max() < 2 ** 24
    xs, ks, dys, idv = dev(cuda, x), dev(cuda, k), dev(cuda, dy), _ids_dev(cuda, ids)
    sy = dw_forward(ssd, cuda, x, k, stride, SN)
    assert sy.shape == (cases.K, oh, ow, C) and same_bits(sy, oracle_ops.depthwise3x3(x, k, stride)) and np.abs(sy).max() > 0
    sdx, _ = dw_backward_dev(ssd, cuda, xs, ks, dys, stride, entry=SN)
    want = oracle_ops.depthwise3x3(bref.dilate_E(dy, H, W, stride), bref.flip(k), 1)
    assert same_bits(sdx.cpu().numpy(), want) and not np.isnan(want).any() and np.abs(want).max() > 0
    X = xs[idv]
    assert X.numel() * 4 > 2 ** 32
    OUT = cuda.full((B, oh, ow, C), NAN, device="cuda")
    ssd.train_calls.depthwise_forward(X, ks, OUT, stride, entry=SN)
    bad = frames_same_bits(cuda, OUT, dev(cuda, sy), idv)
    assert bad is None, "out differs from its small frame in frames %d .. (of %d)" % (bad, B)
    del OUT
    DY = dys[idv]
    DX, DW = dw_backward_dev(ssd, cuda, X, ks, DY, stride, entry=SN)
    bad = frames_same_bits(cuda, DX, sdx, idv)
    assert bad is None, "dx differs from its small frame in frames %d .. (of %d)" % (bad, B)
    assert np.array_equal(DW.cpu().numpy().astype(f64), want_dw.astype(f64))


def test_max_pool_gradient_past_4_gib(ssd, cuda):
    """46 000 tiled frames of 32 x 32 x 24: x and dx are 4 521 984 000 bytes each, dy a quarter; 10 GiB of device memory at the peak.
    The frames of the second-pass test's kind: the K-frame dx is the restated tie rule's bit for bit, every frame of the large dx
    has the bits of its small frame."""
    B, H, W, C = sc.C2
    _require_free(cuda, sc.C2_NEED, "max pool")
    X, _ = _tiled_pool(ssd, cuda, B, H, W, C, 81)
    assert X.numel() * 4 > 2 ** 32


def test_the_copies_past_4_gib(ssd, cuda):
    """18 600 000 rows of D = 58 (two words per access): x, y and every half are 4 315 200 000 bytes, past 2^32; the concat's output is
    past 2^33.  Random 32-bit patterns drawn on the device; the shuffle, its transpose, the concat and the split against the plain
    torch restatement (stack(.., -1).reshape, cat, slices) on the raw words on the device, and the last row on the host as well.
    27 GiB of device memory at the peak: six tensors of rows * D words and one comparison's mask of a byte per word."""
    rows, D = sc.C3
    _require_free(cuda, sc.C3_NEED, "copies")
    calls = ssd.train_calls
    gen = cuda.Generator(device="cuda").manual_seed(91)
    XI, YI = (cuda.randint(-2 ** 31, 2 ** 31 - 1, (rows, D), dtype=cuda.int32, device="cuda", generator=gen) for _ in range(2))
    X, Y = XI.view(cuda.float32), YI.view(cuda.float32)
    assert X.numel() * 4 > 2 ** 32 and not cuda.equal(XI[-1], YI[-1]) and int(XI[-1].abs().max()) > 0
    lx, ly = XI[-1].cpu().numpy(), YI[-1].cpu().numpy()
    lz = np.stack([lx, ly], axis=-1).reshape(-1)
    words = lambda t: t.view(cuda.int32)
    same = lambda t, want: bool((words(t) == want).all())
    XO, YO = cuda.full_like(X, NAN), cuda.full_like(Y, NAN)
    calls.shuffle(X, Y, XO, YO)
    Z = cuda.stack([XI, YI], dim=-1).reshape(rows, 2 * D)               # z[2i] = x[i], z[2i+1] = y[i]
    assert same(XO, Z[:, :D]) and same(YO, Z[:, D:])
    assert np.array_equal(words(XO[-1]).cpu().numpy(), lz[:D]) and np.array_equal(words(YO[-1]).cpu().numpy(), lz[D:])
    del Z
    BX, BY = cuda.full_like(X, NAN), cuda.full_like(Y, NAN)
    calls.shuffle(XO, YO, BX, BY, transpose=True)                       # the transpose of the forward gives the inputs back
    assert same(BX, XI) and same(BY, YI)
    assert np.array_equal(words(BX[-1]).cpu().numpy(), lx) and np.array_equal(words(BY[-1]).cpu().numpy(), ly)
    del XO, YO, BX, BY
    OUT = cuda.full((rows, 2 * D), NAN, device="cuda")
    assert OUT.numel() * 4 > 2 ** 33
    calls.concat(X, Y, OUT)
    CAT = cuda.cat([XI, YI], dim=1)
    assert same(OUT, CAT)
    assert np.array_equal(words(OUT[-1]).cpu().numpy(), np.concatenate([lx, ly]))
    del CAT
    SX, SY = cuda.full_like(X, NAN), cuda.full_like(Y, NAN)
    calls.split(OUT, SX, SY)
    assert same(SX, XI) and same(SY, YI)
    assert np.array_equal(words(SX[-1]).cpu().numpy(), lx) and np.array_equal(words(SY[-1]).cpu().numpy(), ly)
