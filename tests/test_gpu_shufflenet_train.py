"""The TRAIN ShuffleNet on the GPU (include/ssd_hip.h, "the TRAIN ShuffleNet"): the depthwise and 1x1 calls at channel counts that
are 2 mod 4 against ssd_depthwise3x3 / ssd_conv2d and the CPU oracle bit for bit and exactly on integers, the batch norm without an
activation against the header's float32 sequence, the shuffle, concat and split as copies of bit patterns, the max pool's gradient
against the restated tie rule, the refusals, TrainableShuffleNet in inference mode against the engine bit for bit and in training
mode against a float64 restatement with forced gates, the FPN's bridge, and the closed loop through a checkpoint."""
import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import head_train_ref as href
from helpers import shufflenet_train_ref as ref
from helpers.backbone_train_gpu import dw_backward_raw, dw_data as _dw_data, dw_exact, loop_closes_through_a_checkpoint
from helpers.head_train_gpu import dev as _dev, same_bits
from helpers.shufflenet_train_gpu import bn_raw as _bn_raw, dw_forward as _dw_forward, pw as _pw
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
B = 2
SN_PARAMS = dict(TINY_PARAMS, backbone="shufflenet")
DW_CASES = [(5, 7, 1), (6, 8, 2), (7, 9, 2)]                          # stride 1; stride 2 with pad_beg 0 and with pad_beg 1


# ----------------------------------------------------------------------------- 1. depthwise
@pytest.mark.parametrize("C", [6, 58, 8])
def test_depthwise_forward_and_data_gradient_bit_for_bit(ssd, cuda, oracle_ops, C):
    """forward = ssd.depthwise3x3 without batch norm (C % 4 == 2: the oracle's depthwise3x3, which that kernel is pinned to -- the
    inference call pads such widths itself), dx = the oracle's depthwise3x3(E, flip(w)); through the C ABI and through autograd."""
    rng = np.random.default_rng(C)
    for h, w, stride in DW_CASES:
        x, k, dy = _dw_data(rng, h, w, C, stride)
        y = _dw_forward(ssd, cuda, x, k, stride, "sn_depthwise")
        assert same_bits(y, oracle_ops.depthwise3x3(x, k, stride)), (h, w, stride)
        assert same_bits(y, ssd.ssd.depthwise3x3(_dev(cuda, x), k, stride).cpu().numpy()) and np.abs(y).max() > 0
        dx, _ = dw_backward_raw(ssd, cuda, x, k, dy, stride, entry="sn_depthwise")
        want = oracle_ops.depthwise3x3(bref.dilate_E(dy, h, w, stride), bref.flip(k), 1)
        assert dx.shape == want.shape and np.array_equal(dx, want) and np.abs(dx).max() > 0, (h, w, stride)
        tx, tk = _dev(cuda, x).requires_grad_(), _dev(cuda, k).requires_grad_()
        ty = ssd.depthwise_conv(tx, tk, stride)
        ty.backward(_dev(cuda, dy))
        assert same_bits(ty.detach().cpu().numpy(), y) and same_bits(tx.grad.cpu().numpy(), dx), (h, w, stride)


@pytest.mark.parametrize("C", [6, 58, 8])
def test_depthwise_weight_gradient_is_exact_on_small_integers(ssd, cuda, C):
    any_nonzero = False
    for h, w, stride in DW_CASES:
        any_nonzero |= bool(np.abs(dw_exact(ssd, cuda, h, w, C, stride, B, C + h * w + stride, entry="sn_depthwise")).max() > 0)
    assert any_nonzero


def test_depthwise_weight_gradient_is_exact_over_several_slabs_at_58_channels(ssd, cuda):
    """C = 58: G = 15 quads, rpp = 17 row lanes, slabs of 136 rows; 2 x 16 x 16 = 512 rows are four slabs, the last partial."""
    rpp, slab_rows, slabs = bref.slab_plan(2 * 16 * 16, 58)
    assert (rpp, slab_rows, slabs) == (17, 136, 4) and 512 % slab_rows
    assert np.abs(dw_exact(ssd, cuda, 16, 16, 58, 1, 2, 99, entry="sn_depthwise")).max() > 0


def test_depthwise_at_8_channels_is_the_old_entry_point_bit_for_bit(ssd, cuda):
    rng = np.random.default_rng(8)
    for h, w, stride in DW_CASES:
        x, k, dy = _dw_data(rng, h, w, 8, stride)
        assert same_bits(_dw_forward(ssd, cuda, x, k, stride, "sn_depthwise"), _dw_forward(ssd, cuda, x, k, stride, "depthwise"))
        new, old = dw_backward_raw(ssd, cuda, x, k, dy, stride, entry="sn_depthwise"), dw_backward_raw(ssd, cuda, x, k, dy, stride, entry="depthwise")
        assert same_bits(new[0], old[0]) and same_bits(new[1], old[1]) and np.abs(old[1]).max() > 0


# ----------------------------------------------------------------------------- 2. pointwise
@pytest.mark.parametrize("Cin,Cout", [(6, 10), (58, 58), (24, 58), (8, 16)])
def test_pointwise_forward_and_gradients(ssd, cuda, oracle_ops, Cin, Cout):
    """forward = ssd.conv2d, dx = the oracle's conv2d(dy, w') bit for bit; dw exact on small integers; through autograd the same."""
    rng = np.random.default_rng(Cin * 7 + Cout)
    h, w = 5, 7
    x, dy = rng.normal(0, 1, (B, h, w, Cin)).astype(f32), rng.normal(0, 1, (B, h, w, Cout)).astype(f32)
    k = rng.normal(0, 0.1, (1, 1, Cin, Cout)).astype(f32)
    y, dx, dw = _pw(ssd, cuda, x, k, dy, "sn_pointwise")
    assert same_bits(y, ssd.ssd.conv2d(_dev(cuda, x), k).cpu().numpy()) and np.abs(y).max() > 0
    want = oracle_ops.conv2d(dy, np.ascontiguousarray(k.transpose(0, 1, 3, 2)))
    assert dx.shape == want.shape and np.array_equal(dx, want) and np.abs(dx).max() > 0
    tx, tk = _dev(cuda, x).requires_grad_(), _dev(cuda, k).requires_grad_()
    ty = ssd.pointwise_conv(tx, tk)
    ty.backward(_dev(cuda, dy))
    assert same_bits(ty.detach().cpu().numpy(), y) and same_bits(tx.grad.cpu().numpy(), dx) and same_bits(tk.grad.cpu().numpy(), dw)
    xi, dyi = rng.integers(-3, 4, x.shape).astype(f32), rng.integers(-3, 4, dy.shape).astype(f32)
    _, _, dwi = _pw(ssd, cuda, xi, k, dyi, "sn_pointwise")
    wanti = np.einsum("bhwi,bhwo->io", xi.astype(f64), dyi.astype(f64))
    assert np.abs(wanti).max() < 2 ** 24 and np.array_equal(dwi.reshape(Cin, Cout).astype(f64), wanti) and np.abs(wanti).max() > 0
    if Cin % 4 == 0:                                                    # the old calls' bits
        yo, dxo, dwo = _pw(ssd, cuda, x, k, dy, "pointwise")
        assert same_bits(y, yo) and same_bits(dx, dxo) and same_bits(dw, dwo)


# ----------------------------------------------------------------------------- 3. the batch norm without an activation
def _bn_inputs(rng, rows, C):
    # gamma 2 .. 4: y = gamma * xhat + beta goes a few percent beyond 6
    return (rng.normal(0.3, 1.5, (rows, C)).astype(f32), rng.uniform(2.0, 4.0, C).astype(f32), rng.normal(0, 0.3, C).astype(f32),
            rng.normal(0, 0.1, C).astype(f32), rng.uniform(0.5, 1.5, C).astype(f32), rng.normal(0, 1, (rows, C)).astype(f32))


@pytest.mark.parametrize("C", [6, 58, 24])
def test_batch_norm_without_activation_is_the_headers_float32_sequence_bit_for_bit(ssd, cuda, C):
    """rows = 3 slabs and a part of one.  The statistics do not depend on the activation: they have the bits of the ReLU call's, which
    the TRAIN head's tests pin to the header; out, dx against the float32 sequence on the kernel's own statistics, dgamma and dbeta."""
    rpp, slab_rows, _ = href.slab_plan([1], C)
    rows = 3 * slab_rows + rpp + 1
    assert href.slab_plan([rows], C)[2] == 4 and rows % slab_rows
    x, gamma, beta, mm, mv, dy = _bn_inputs(np.random.default_rng(C), rows, C)
    g = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy)
    relu = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, act="relu", entry="bn_act")
    for name in ("mean", "var", "invstd", "mm", "mv"):
        assert same_bits(g[name], relu[name]), name
    assert same_bits(g["invstd"], href.invstd_f32(g["var"])) and np.all(np.abs(g["mean"] - x.mean(0)) < 1e-5)
    wm, wv = href.moving_update(mm, mv, g["mean"], g["var"], rows)
    assert same_bits(g["mm"], wm) and same_bits(g["mv"], wv) and not same_bits(g["mm"], mm)
    y, dx = ref.bn_none_f32(x, gamma, beta, g["mean"], g["invstd"], dy, g["dgamma"], g["dbeta"])
    assert same_bits(g["y"], y) and (y < 0).any() and (y > 6).any()                     # nothing is clipped
    assert same_bits(g["dx"], dx) and np.abs(dx).max() > 0
    xhat = ((x - g["mean"]) * g["invstd"]).astype(f32).astype(f64)
    # dgamma, dbeta: double column sums rounded once.  The project's statement for them (head_train_ref.double_sum_bound, as in the
    # ReLU6 test) holds for ANY order of the double additions, the header's slab order included: about one float32 ulp around the exact
    # sum.  Two calls give the same bits (below).
    for name, terms in (("dbeta", dy.astype(f64)), ("dgamma", dy.astype(f64) * xhat)):  # g = dy: every gate is open
        want, tol = href.double_sum_bound(terms)
        assert np.all(np.abs(g[name].astype(f64) - want.astype(f64)) <= tol), name
    again = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy)
    for name in g:
        assert same_bits(g[name], again[name]), name
    # through autograd: the same bits
    tx, tg, tb = (_dev(cuda, v).requires_grad_() for v in (x, gamma, beta))
    ty = ssd.batch_norm_act(tx, tg, tb, _dev(cuda, mm), _dev(cuda, mv), training=True, act="none")
    ty.backward(_dev(cuda, dy))
    assert same_bits(ty.detach().cpu().numpy(), g["y"]) and same_bits(tx.grad.cpu().numpy(), g["dx"])
    assert same_bits(tg.grad.cpu().numpy(), g["dgamma"]) and same_bits(tb.grad.cpu().numpy(), g["dbeta"])


@pytest.mark.parametrize("C", [6, 58])
def test_batch_norm_relu_through_the_new_entry_points_is_the_old_pair_bit_for_bit(ssd, cuda, C):
    x, gamma, beta, mm, mv, dy = _bn_inputs(np.random.default_rng(C + 2), 442, C)
    for act in ("relu", "relu6"):
        old = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy, act=act, entry="bn_act")
        new = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy, act=act, entry="sn_bn")
        for name in old:
            assert same_bits(old[name], new[name]), (act, name)
        assert np.isfinite(old["dx"]).all() and old["y"].min() == 0
    none = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy)
    assert none["y"].min() < 0 and not same_bits(none["dx"], old["dx"])


@pytest.mark.parametrize("C", [6, 58])
def test_batch_norm_without_activation_inference_form_is_the_oracles_epilogue(ssd, cuda, oracle_ops, C):
    x, gamma, beta, mm, mv, _ = _bn_inputs(np.random.default_rng(C + 3), 442, C)
    g = _bn_raw(ssd, cuda, x, gamma, beta, mm, mv, training=0)
    want = oracle_ops.bn_act(x, gamma, beta, mm, mv, None)
    assert same_bits(g["y"], want) and want.min() < 0
    assert same_bits(g["mm"], mm) and same_bits(g["mv"], mv) and np.isnan(g["mean"]).all()
    ty = ssd.batch_norm_act(_dev(cuda, x), *[_dev(cuda, v) for v in (gamma, beta, mm, mv)], training=False, act="none")
    assert same_bits(ty.cpu().numpy(), want)


# ----------------------------------------------------------------------------- 4. shuffle, concat, split
def _planted(rng, rows, D):
    """Random bit patterns with NaN payloads, infinities, denormals and -0 planted."""
    a = rng.normal(0, 1, (rows, D)).astype(f32)
    flat = a.reshape(-1).view(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000], np.uint32)
    idx = rng.choice(flat.size, min(flat.size, 64), replace=False)
    flat[idx] = special[np.arange(idx.size) % special.size]
    return a


def _bits_dev(cuda, t):
    return t.contiguous().view(cuda.int32).cpu().numpy()


def _from_bits(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda().view(cuda.float32)


def _copies(ssd, cuda, oracle_ops, x, y):
    """All four copies on bit patterns x, y [rows, D] against the oracle and numpy; every comparison on the raw words."""
    calls = ssd.train_calls
    X, Y = _from_bits(cuda, x), _from_bits(cuda, y)
    XO, YO = cuda.full_like(X, 3.0), cuda.full_like(Y, 3.0)
    calls.shuffle(X, Y, XO, YO)
    bx, by = x.view(np.int32), y.view(np.int32)
    z = np.stack([bx, by], axis=-1).reshape(x.shape[0], -1)
    D = x.shape[1]
    assert np.array_equal(_bits_dev(cuda, XO), z[:, :D]) and np.array_equal(_bits_dev(cuda, YO), z[:, D:])
    BX, BY = cuda.full_like(X, 3.0), cuda.full_like(Y, 3.0)
    calls.shuffle(XO, YO, BX, BY, transpose=True)                       # the transpose of the forward gives the inputs back
    assert np.array_equal(_bits_dev(cuda, BX), bx) and np.array_equal(_bits_dev(cuda, BY), by)
    OUT = cuda.full((x.shape[0], 2 * D), 3.0, device="cuda")
    calls.concat(X, Y, OUT)
    assert np.array_equal(_bits_dev(cuda, OUT), np.concatenate([bx, by], axis=1))
    SX, SY = cuda.full_like(X, 3.0), cuda.full_like(Y, 3.0)
    calls.split(OUT, SX, SY)
    assert np.array_equal(_bits_dev(cuda, SX), bx) and np.array_equal(_bits_dev(cuda, SY), by)
    return XO, YO


@pytest.mark.parametrize("D", [1, 2, 24, 58])
def test_shuffle_concat_and_split_are_copies_of_bit_patterns(ssd, cuda, oracle_ops, D):
    rng = np.random.default_rng(D)
    x, y = _planted(rng, 777, D), _planted(rng, 777, D)
    XO, YO = _copies(ssd, cuda, oracle_ops, x, y)
    ox, oy = oracle_ops.concat_shuffle_split(x, y)
    assert np.array_equal(_bits_dev(cuda, XO), ox.view(np.int32)) and np.array_equal(_bits_dev(cuda, YO), oy.view(np.int32))
    # through autograd: the forward's bits, and the gradients are the transposes
    tx, ty = _from_bits(cuda, np.nan_to_num(x)).requires_grad_(), _from_bits(cuda, np.nan_to_num(y)).requires_grad_()
    a, b = ssd.concat_shuffle_split(tx, ty)
    da, db = rng.normal(0, 1, (777, D)).astype(f32), rng.normal(0, 1, (777, D)).astype(f32)
    cuda.autograd.backward([a, b], [_dev(cuda, da), _dev(cuda, db)])
    wx, wy = ref.shuffle_transpose(da, db)
    assert same_bits(tx.grad.cpu().numpy(), wx) and same_bits(ty.grad.cpu().numpy(), wy)
    tx2, ty2 = tx.detach().clone().requires_grad_(), ty.detach().clone().requires_grad_()
    dc = rng.normal(0, 1, (777, 2 * D)).astype(f32)
    ssd.concat_channels(tx2, ty2).backward(_dev(cuda, dc))
    assert same_bits(tx2.grad.cpu().numpy(), dc[:, :D]) and same_bits(ty2.grad.cpu().numpy(), dc[:, D:])


@pytest.mark.parametrize("D", [58, 24, 1, 122])
def test_the_copies_go_round_their_grid_more_than_once(ssd, cuda, oracle_ops, D):
    """58 and 122: two words per access, 24: four, 1: one -- every instance of sn_copy_kernel past one pass of its capped grid."""
    rows = ref.copy_rows_past_one_grid_pass(D)
    rng = np.random.default_rng(D + 1)
    x = rng.integers(0, 2 ** 32, (rows, D), dtype=np.uint64).astype(np.uint32).view(f32)
    y = rng.integers(0, 2 ** 32, (rows, D), dtype=np.uint64).astype(np.uint32).view(f32)
    _copies(ssd, cuda, oracle_ops, x, y)


# ----------------------------------------------------------------------------- 5. the max pool's gradient
def _pool_grad(ssd, cuda, x, dy):
    X, DY = _from_bits(cuda, x), _dev(cuda, dy)
    DX = cuda.full_like(X, float("nan"))
    ssd.train_calls.maxpool_backward(X, DY, DX)
    return DX.cpu().numpy()


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("h,w", [(4, 6), (8, 8)])
def test_max_pool_gradient_is_the_restated_tie_rule_bit_for_bit(ssd, cuda, C, h, w):
    rng = np.random.default_rng(C + h)
    x = np.maximum(rng.normal(0, 1, (B, h, w, C)), 0).astype(f32)       # ReLU-like: about half the taps are tied at zero
    x[0, :, :, 1] = np.nan                                              # every window of this channel is all NaN: no winner
    x[1, :3, :3, 2] = np.nan                                            # one all-NaN window beside mixed ones
    dy = rng.normal(0, 1, (B, h // 2, w // 2, C)).astype(f32)
    assert (x == 0).sum() > x.size // 4
    got, want = _pool_grad(ssd, cuda, x, dy), ref.maxpool_grad(x, dy)
    assert same_bits(got, want) and np.abs(want).max() > 0
    assert np.all(got[0, :, :, 1] == 0) and got[1, 0, 0, 2] == 0
    assert same_bits(ssd.ssd.maxpool3x3s2(_from_bits(cuda, x)).cpu().numpy()[:, :, :, 3:], ref.maxpool_forward(x)[:, :, :, 3:])
    # tie-free data, integer dy: torch autograd, exactly, and through this project's autograd Function
    xt = (rng.permutation(B * h * w * C).astype(f32) - f32(B * h * w * C // 2)).reshape(B, h, w, C)
    dyi = rng.integers(-4, 5, dy.shape).astype(f32)
    _, dxt = ref.torch_maxpool(xt, dyi)
    assert np.array_equal(_pool_grad(ssd, cuda, xt, dyi).astype(f64), dxt)
    tx = _dev(cuda, xt).requires_grad_()
    ssd.maxpool3x3s2_train(tx).backward(_dev(cuda, dyi))
    assert np.array_equal(tx.grad.cpu().numpy().astype(f64), dxt)


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_come_before_any_launch(ssd, cuda):
    L = ssd.lib()
    H, W, C = 6, 8, 58
    full = lambda *shape: cuda.full(shape, 7.0, device="cuda")
    zero = lambda *shape: cuda.zeros(shape, device="cuda")
    x, w, dy1 = zero(B, H, W, C), zero(3, 3, C, 1), zero(B, H, W, C)
    out, dx, dw = full(B, H, W, C), full(B, H, W, C), full(3, 3, C, 1)
    ws = cuda.empty(1 << 20, dtype=cuda.uint8, device="cuda")
    s = ssd.train_calls.stream(x.device)
    err = lambda: L.ssd_last_error().decode()
    fwd = lambda c=C, stride=1, xp=x.data_ptr(): L.ssd_sn_depthwise_train_forward(xp, B, H, W, c, w.data_ptr(), stride, out.data_ptr(), s)
    need = L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, C, 1)
    bwd = lambda c=C, wsb=need, dyp=dy1.data_ptr(): L.ssd_sn_depthwise_train_backward(x.data_ptr(), dyp, B, H, W, c, w.data_ptr(), 1, dx.data_ptr(),
                                                                                      dw.data_ptr(), ws.data_ptr(), wsb, s)
    assert 0 < need <= ws.numel()
    assert fwd(c=57) == -1 and "even" in err() and bwd(c=57) == -1 and fwd(stride=3) == -1
    assert bwd(wsb=need - 1) == -1 and "workspace too small" in err()
    assert fwd(xp=x.data_ptr() + 8) == -1 and bwd(dyp=dy1.data_ptr() + 8) == -1 and "16-byte" in err()
    # the batch norm
    Lv = ssd._lib.SsdBnLevel
    vec = [zero(C + 2)[:C] for _ in range(9)]
    x2, y2 = x.view(-1, C), out.view(-1, C)
    lv = (Lv * 1)(Lv(x2.shape[0], x2.data_ptr(), x2.data_ptr(), y2.data_ptr(), *[v.data_ptr() for v in vec]))
    bn = lambda act: L.ssd_sn_bn_train_forward(lv, 1, C, act, 1, 1e-3, 0.007, ws.data_ptr(), ws.numel(), s)
    assert bn(3) == -1 and "act" in err()
    assert L.ssd_sn_bn_train_backward(lv, 1, C, 3, ws.data_ptr(), ws.numel(), s) == -1 and "act" in err()
    # the 1x1 convolution
    CL = ssd._lib.SsdConvLevel
    Cout = 10
    dyc, wc, dwc, yc = zero(B, H, W, Cout), zero(1, 1, C, Cout), full(1, 1, C, Cout), full(B, H, W, Cout)
    clv = lambda o: (CL * 1)(CL(H, W, x.data_ptr(), dyc.data_ptr(), o))
    pneed = L.ssd_sn_pointwise_train_workspace_bytes(clv(dx.data_ptr()), 1, B, C, Cout)
    assert 0 < pneed <= ws.numel() and L.ssd_sn_pointwise_train_workspace_bytes(clv(dx.data_ptr()), 1, B, 57, Cout) == 0
    pwf = lambda wsb: L.ssd_sn_pointwise_train_forward(clv(yc.data_ptr()), 1, B, C, Cout, wc.data_ptr(), ws.data_ptr(), wsb, s)
    pwb = lambda o, wsb: L.ssd_sn_pointwise_train_backward(clv(o), 1, B, C, Cout, wc.data_ptr(), dwc.data_ptr(), ws.data_ptr(), wsb, s)
    assert pwf(pneed - 1) == -1 and pwb(dx.data_ptr(), pneed - 1) == -1 and "workspace too small" in err()
    assert pwb(dx.data_ptr() + 8, pneed) == -1 and "16-byte" in err()
    # the copies and the max pool
    a, b, xo, yo, cat = zero(12, C), zero(12, C), full(12, C), full(12, C), full(12, 2 * C)
    sh = lambda rows=12, D=C, xop=xo.data_ptr(): L.ssd_sn_shuffle_train(a.data_ptr(), b.data_ptr(), rows, D, 0, xop, yo.data_ptr(), s)
    assert sh(rows=0) == -1 and "rows" in err() and sh(D=0) == -1 and sh(xop=xo.data_ptr() + 4) == -1 and "16-byte" in err()
    assert sh(xop=a.data_ptr()) == -1 and "overlap" in err()
    assert L.ssd_sn_concat_train(a.data_ptr(), b.data_ptr(), 0, C, cat.data_ptr(), s) == -1 and "rows" in err()
    assert L.ssd_sn_split_train(cat.data_ptr(), 12, C, xo.data_ptr(), xo.data_ptr(), s) == -1 and "overlap" in err()
    px, pdy, pdx = zero(B, H, W, 8), zero(B, H // 2, W // 2, 8), full(B, H, W, 8)
    mp = lambda h=H, c=8: L.ssd_sn_maxpool_train_backward(px.data_ptr(), pdy.data_ptr(), B, h, W, c, pdx.data_ptr(), s)
    assert mp(h=5) == -1 and "even" in err() and mp(c=6) == -1
    cuda.cuda.synchronize()
    for t in (out, dx, dw, dwc, yc, xo, yo, cat, pdx):                  # nothing ran
        assert bool((t == 7.0).all())
    # and the same calls with good arguments run
    assert fwd() == 0 and bwd() == 0 and bn(0) == 0 and pwf(pneed) == 0 and pwb(dx.data_ptr(), pneed) == 0 and sh() == 0 and mp() == 0
    assert L.ssd_sn_concat_train(a.data_ptr(), b.data_ptr(), 12, C, cat.data_ptr(), s) == 0
    cuda.cuda.synchronize()
    for t in (out, dx, dw, dwc, yc, xo, yo, cat, pdx):
        assert bool((t == 0).all())


# ----------------------------------------------------------------------------- 7. inference mode
def _engine(ssd, cuda, params, seed, size=128):
    W = ssd.synthetic_weights(params, seed=seed, logits_bias=-4.0)
    img = np.random.default_rng(seed + 1).integers(0, 256, (B, size, size, 3), dtype=np.uint8)
    eng = ssd.Engine(params, W, device=0)
    eng.forward(cuda.from_numpy(img).cuda())
    kept = {k: eng.get_tensor(k) for k in ("c3", "c4", "c5")}
    eng.close()
    return W, img, kept


@pytest.mark.parametrize("depth", [1.0, 0.5])
def test_trainable_shufflenet_in_inference_mode_is_the_engine_bit_for_bit(ssd, cuda, depth):
    params = dict(SN_PARAMS, depth_multiplier=depth)
    W, img, kept = _engine(ssd, cuda, params, 31)
    d0 = {1.0: 116, 0.5: 48}[depth]
    for train_first in (False, True):
        m = ssd.TrainableShuffleNet(params, W, device="cuda", keep_features=True, train_first=train_first).eval()
        with cuda.no_grad():
            cs = m(cuda.from_numpy(img).cuda())
        assert [tuple(c.shape[1:]) for c in cs] == [(16, 16, d0), (8, 8, 2 * d0), (4, 4, 1024)]
        for name, c in zip(("c3", "c4", "c5"), cs):
            assert np.array_equal(c.cpu().numpy(), kept[name]) and np.abs(kept[name]).max() > 0, (name, train_first)
        assert len(m.features) == 55 + 4 + (1 if train_first else 0) and cuda.equal(m.features["Conv5"], cs[2])   # + MaxPool, Stage2 .. 4
        assert cuda.equal(m.features["Stage2"], cs[0]) and m.features["MaxPool"].shape[1:] == (32, 32, 24)
        for k, v in m.statistics().items():                             # inference mode moves nothing
            assert same_bits(v.cpu().numpy(), W[k]), k
    with pytest.raises(ValueError, match="32"):
        m(cuda.zeros((1, 144, 128, 3), dtype=cuda.uint8, device="cuda"))


# ----------------------------------------------------------------------------- 8. training mode
def test_trainable_shufflenet_in_training_mode_against_the_float64_restatement(ssd, cuda):
    """The whole backbone from the uint8 frames with train_first=True, all 56 batch norms on batch statistics: c3, c4, c5, the
    gradient of sum(c_l * d_l) (d_l random, both signs) with respect to 149 of the 168 variables, and the 112 moving statistics, per
    tensor and norm-wise (head_train_ref.rel) against a float64 CPU torch restatement: 264 comparisons.  The other 19 variables are the
    betas of the depthwise batch norms, whose gradient is ZERO in exact arithmetic (a per-channel constant that a bias-free 1x1
    convolution carries into a batch norm on batch statistics, which subtracts it): a ratio of two rounding residues says nothing, so
    for them |d beta| is bounded by (K + 16) 2^-24 times the absolute sum of its terms (shufflenet_train_ref.dead_beta_bound, where the
    reasoning is), and the float64 run must stay below 2^-24 of that bound.  A ReLU gate that flips between two precisions moves
    the lower layers' gradients far more than rounding does, so the restatement takes its gates from the run under test (layer by
    layer out = y * open, open read from the module's features); the gates themselves are pinned by the bit-for-bit batch-norm tests.
    The gradients of Conv1 reach through the max pool; its ties at zero sit behind closed ReLU gates, so the tie rule cannot move
    them.  Bound: the kernels' figure may be at most FACTOR = 4 x the figure of a float32 CPU torch run with the same forced gates,
    the project's margin for the same quantities in the head, FPN and MobileNet tests.  Every ratio and the worst one are printed.
    Measured on an MI355X (profiles/r25_shufflenet_train.log): gates 453 693 open, 448 451 closed; the worst ratios are 1.69 x (d
    Stage4/unit_2/conv1x1_before/batch_norm/gamma: 2.23e-5 against 1.32e-5), 1.66 x (d Stage2/unit_1/depthwise/batch_norm/gamma) and
    1.65 x (d Stage4/unit_4/depthwise/batch_norm/gamma; Stage4/unit_1/second_branch/depthwise moving variance); c3, c4, c5 1.07, 1.16
    and 0.99 x; d Conv1/weights 0.71 x.  The 19 zero gradients: the kernels' |d beta| is at most 0.0020 of its bound (d
    Stage4/unit_1/depthwise/batch_norm/beta), the float32 torch run's 0.0020, the float64 run's 4.1e-12."""
    import torch
    FACTOR = 4.0
    W = ssd.synthetic_weights(SN_PARAMS, seed=41, logits_bias=-4.0)
    img = np.random.default_rng(42).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    m = ssd.TrainableShuffleNet(SN_PARAMS, W, device="cuda", keep_features=True, train_first=True).train()
    rng = np.random.default_rng(43)
    ds = [rng.normal(0, 1, (B, h, h, c)).astype(f32) for h, c in ((16, 116), (8, 232), (4, 1024))]
    cs = m(cuda.from_numpy(img).cuda())
    cuda.autograd.backward(cs, [_dev(cuda, d) for d in ds])
    feats = {k: v.cpu().numpy() for k, v in m.features.items()}
    gates = ref.gates_of(feats)
    kinds = [sum(int(g.sum()) for g in gates.values()), sum(int((~g).sum()) for g in gates.values())]
    print("shufflenet train mode gates: open %d, closed %d" % tuple(kinds))
    assert len(gates) == 56 - 19 and all(kinds)                         # 37 ReLU layers (19 depthwise have none); open and closed gates occur
    runs = {}
    for dtype in (torch.float64, torch.float32):
        outs, T, S, raw = ref.torch_shufflenet(W, img, dtype, gates)
        torch.autograd.backward(outs, [torch.tensor(d.astype(f64), dtype=dtype) for d in ds])
        if dtype == torch.float64:
            dead = {"d " + n: ref.dead_beta_bound(W, raw, n) for n in ref.dead_betas(T)}
        rows = [("c%d" % (3 + l), outs[l].detach().numpy()) for l in range(3)]
        rows += [("d " + k, v.grad.numpy()) for k, v in T.items()] + [(k, v.numpy()) for k, v in S.items()]
        runs[dtype] = dict(rows)
    got = {"c%d" % (3 + l): cs[l].detach().cpu().numpy() for l in range(3)}
    got.update({"d " + k: v.grad.cpu().numpy() for k, v in m.named_variables().items()})
    got.update({k: v.cpu().numpy() for k, v in m.statistics().items()})
    assert set(got) == set(runs[torch.float64]) and len(got) == 3 + 168 + 112            # 264 compared by ratio + the 19 zero gradients
    assert len(dead) == 19 and set(dead) <= set(got)
    bad, worst, dead_worst = [], (0.0, None), (0.0, None)
    for name, bound in dead.items():                                    # zero in exact arithmetic: small against the scale of its terms
        assert np.all(bound > 0), name
        frac = [float((np.abs(v) / bound).max()) for v in (runs[torch.float64][name], runs[torch.float32][name], got[name])]
        print("shufflenet train mode %-64s ZERO: |d beta| / bound  float64 torch %.3g  float32 torch %.3g  kernels %.3g" % ((name,) + tuple(frac)))
        dead_worst = max(dead_worst, (frac[2], name))
        assert frac[0] <= 2.0 ** -24, name                              # the float64 run confirms the zero far below the float32 bound
        if not frac[2] <= 1.0:
            bad.append((name, frac[2], 1.0))
    print("shufflenet train mode worst |d beta| / bound of the 19 zero gradients %.3g (%s)" % dead_worst)
    for name, r64 in runs[torch.float64].items():
        if name in dead:
            continue
        yard, d = ref.rel(runs[torch.float32][name], r64), ref.rel(got[name], r64)
        # no vacuous comparison: the float64 value stands far above what float32 arithmetic leaves of it (a quantity that is zero but
        # for rounding, like the 19 above, has a yardstick of 1e8)
        assert np.abs(r64).max() > 0 and 0 < yard <= 1e-3, (name, yard)
        print("shufflenet train mode %-64s float32 torch %.3g  kernels %.3g  ratio %.2f" % (name, yard, d, d / yard))
        worst = max(worst, (d / yard, name))
        if not d <= FACTOR * yard:
            bad.append((name, d, yard))
    print("shufflenet train mode worst ratio %.2f (%s)" % worst)
    assert not bad, bad
    for k, v in m.statistics().items():
        assert not np.array_equal(v.cpu().numpy(), W[k]), k


# ----------------------------------------------------------------------------- 9. the bridge through the FPN
def test_gradients_flow_from_the_fpn_into_the_backbone(ssd, cuda):
    W = ssd.synthetic_weights(SN_PARAMS, seed=13, logits_bias=-4.0)
    img = cuda.from_numpy(np.random.default_rng(14).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)).cuda()
    backbone = ssd.TrainableShuffleNet(SN_PARAMS, W, device="cuda").train()
    fpn = ssd.TrainableFPN(SN_PARAMS, W, device="cuda").train()
    cs = backbone(img)
    assert [c.shape[3] for c in cs] == [116, 232, 1024] and all(c.requires_grad for c in cs)
    for c in cs:
        c.retain_grad()
    rng = np.random.default_rng(15)
    ds = [_dev(cuda, rng.normal(0, 1, (B, h, h, 256)).astype(f32)) for h in (16, 8, 4, 2, 1)]
    cuda.autograd.backward(fpn(cs), ds)
    for c in cs:
        assert c.grad is not None and bool(cuda.isfinite(c.grad).all()) and float(c.grad.abs().max()) > 0
    dead = ref.dead_betas(backbone.named_variables())                   # zero in exact arithmetic: nothing flows there (see the test above)
    assert len(dead) == 19
    for name, p in backbone.named_variables().items():
        assert p.grad is not None and bool(cuda.isfinite(p.grad).all()), name
        assert name in dead or float(p.grad.abs().max()) > 0, name


# ----------------------------------------------------------------------------- 10. the loop
def test_the_loop_closes_through_a_checkpoint(ssd, cuda, tmp_path):
    """images -> TrainableShuffleNet -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward -> one TrainStep over
    the three modules' variables with Conv1 frozen -> save -> a fresh Detector on that checkpoint."""
    def dead_betas(variables):                                          # the depthwise batch norms' betas: their gradient is zero
        dead = ref.dead_betas(variables)
        assert len(dead) == 19
        return dead
    loop_closes_through_a_checkpoint(ssd, cuda, tmp_path, ssd.TrainableShuffleNet, SN_PARAMS, "ShuffleNetV2/Conv1/", dead_betas, "c3")
