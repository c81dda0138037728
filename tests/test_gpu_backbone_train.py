"""The TRAIN backbone on the GPU (include/ssd_hip.h, "the TRAIN backbone"): the raw depthwise forward against ssd_depthwise3x3 and
its data gradient against the CPU oracle bit for bit, its weight gradient exactly on integers and within the bound of a double sum
rounded once on random data, the 1x1 data gradient against the oracle bit for bit, the batch norm with ReLU6 against the header's
float32 sequence, the refusals, TrainableMobileNet in inference mode against the engine bit for bit and in training mode against a
float64 restatement with forced gates, the FPN's bridge to c3, c4, c5, and the closed loop through a checkpoint."""
import numpy as np
import pytest

from helpers import backbone_train_ref as ref
from helpers import head_train_ref as href
from helpers.backbone_train_gpu import (dw_backward_raw as _dw_backward_raw, dw_data as _dw_data, dw_exact as _dw_exact,
                                        loop_closes_through_a_checkpoint)
from helpers.head_train_gpu import bn_raw, conv_backward, dev as _dev, same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
B = 2
SIZES = [(6, 8), (5, 7), (13, 17), (1, 1), (2, 2)]                    # 13 x 17 leaves remainders in every thread's 2 x 4 patch
WIDTHS = [4, 36, 1024]


# ----------------------------------------------------------------------------- 1. the depthwise forward
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", WIDTHS)
def test_depthwise_forward_is_ssd_depthwise3x3_bit_for_bit(ssd, cuda, C, stride):
    rng = np.random.default_rng(C + stride)
    for h, w in SIZES:
        x, k, _ = _dw_data(rng, h, w, C, stride)
        y = ssd.depthwise_conv(_dev(cuda, x), _dev(cuda, k), stride)
        want = ssd.ssd.depthwise3x3(_dev(cuda, x), k, stride)
        assert tuple(y.shape) == (B,) + ref.dw_out_hw(h, w, stride) + (C,)
        assert y.shape == want.shape and cuda.equal(y, want) and float(want.abs().max()) > 0, (h, w)


# ----------------------------------------------------------------------------- 2. the depthwise data gradient
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", WIDTHS)
def test_depthwise_data_gradient_is_the_oracles_convolution_of_E_bit_for_bit(ssd, cuda, oracle_ops, C, stride):
    """dx = depthwise3x3(E, flip(w), stride 1) of the CPU oracle, E the zero-dilated dy of the header (never materialised on the
    GPU); through the C ABI and, with the same bits, through autograd."""
    rng = np.random.default_rng(C * 3 + stride)
    for h, w in SIZES:
        x, k, dy = _dw_data(rng, h, w, C, stride)
        dx, _ = _dw_backward_raw(ssd, cuda, x, k, dy, stride)
        want = oracle_ops.depthwise3x3(ref.dilate_E(dy, h, w, stride), ref.flip(k), 1)
        assert dx.shape == want.shape and np.array_equal(dx, want), (h, w)
        assert np.abs(dx).max() > 0
        tx, tk = _dev(cuda, x).requires_grad_(), _dev(cuda, k).requires_grad_()
        ssd.depthwise_conv(tx, tk, stride).backward(_dev(cuda, dy))
        assert same_bits(tx.grad.cpu().numpy(), dx), (h, w)


# ----------------------------------------------------------------------------- 3. the depthwise weight gradient
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", WIDTHS)
def test_depthwise_weight_gradient_is_exact_on_small_integers(ssd, cuda, C, stride):
    any_nonzero = False
    for h, w in SIZES:
        any_nonzero |= bool(np.abs(_dw_exact(ssd, cuda, h, w, C, stride, B, C + h * w + stride)).max() > 0)
    assert any_nonzero


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_weight_gradient_is_exact_over_several_slabs(ssd, cuda, stride):
    """C = 32: rpp = 32 row lanes, slabs of 256 rows.  B = 3 on 13 x 17: 663 output rows at stride 1 are three slabs, the last
    partial; at stride 2, 31 x 33 -> 16 x 17 x 3 = 816 rows are four."""
    h, w = (13, 17) if stride == 1 else (31, 33)
    oh, ow = ref.dw_out_hw(h, w, stride)
    rpp, slab_rows, slabs = ref.slab_plan(3 * oh * ow, 32)
    assert (rpp, slab_rows) == (32, 256) and slabs >= 3 and (3 * oh * ow) % slab_rows
    assert np.abs(_dw_exact(ssd, cuda, h, w, 32, stride, 3, 77 + stride)).max() > 0


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [36, 1024])
def test_depthwise_weight_gradient_obeys_the_bound_of_a_double_sum_rounded_once(ssd, cuda, C, stride):
    """|dw - fl32(exact sum)| <= n 2^-53 sum|term| + one float32 ulp per element (head_train_ref.double_sum_bound, the bound of the
    batch norm's dgamma): the products are exact in double, so only the order of the double additions and one rounding remain."""
    rng = np.random.default_rng(C + 10 * stride)
    for h, w in [(13, 17), (5, 7)]:
        x, k, dy = _dw_data(rng, h, w, C, stride)
        terms = ref.dw_terms(x, dy, stride)
        _, dw = _dw_backward_raw(ssd, cuda, x, k, dy, stride, with_dx=False)
        worst = 0.0
        for t in range(9):
            want, tol = href.double_sum_bound(terms[:, t, :])
            err = np.abs(dw.reshape(9, C)[t].astype(f64) - want.astype(f64))
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (h, w, t, float((err / tol).max()))
        print("depthwise dw C=%d s=%d %dx%d: worst |dw - exact| / bound = %.3g" % (C, stride, h, w, worst))
        assert np.isfinite(dw).all() and np.abs(dw).max() > 0
        _, dw2 = _dw_backward_raw(ssd, cuda, x, k, dy, stride, with_dx=False)
        assert same_bits(dw, dw2)


# ----------------------------------------------------------------------------- 4. the 1x1 data gradient
@pytest.mark.parametrize("Cin,Cout", [(8, 256), (116, 256), (1024, 32), (256, 24)])
def test_pointwise_data_gradient_is_the_oracles_convolution_bit_for_bit(ssd, cuda, oracle_ops, Cin, Cout):
    """dx = conv2d(dy, w'), w'[0,0,co,ci] = w[0,0,ci,co], two levels in one call; dw has the bits of ssd_conv_train_backward."""
    rng = np.random.default_rng(Cin * 7 + Cout)
    sizes = [(5, 7), (3, 4)]
    xs = [rng.normal(0, 1, (B, h, w, Cin)).astype(f32) for h, w in sizes]
    dys = [rng.normal(0, 1, (B, h, w, Cout)).astype(f32) for h, w in sizes]
    k = rng.normal(0, 0.05, (1, 1, Cin, Cout)).astype(f32)
    tx, tk = [_dev(cuda, x).requires_grad_() for x in xs], _dev(cuda, k).requires_grad_()
    ys = ssd.pointwise_conv(tx, tk)
    for x, y in zip(xs, ys):
        assert cuda.equal(y.detach(), ssd.ssd.conv2d(_dev(cuda, x), k))
    cuda.autograd.backward(ys, [_dev(cuda, d) for d in dys])
    kt = np.ascontiguousarray(k.transpose(0, 1, 3, 2))
    for dy, t in zip(dys, tx):
        want = oracle_ops.conv2d(dy, kt)
        got = t.grad.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want) and np.abs(want).max() > 0
    _, dw, _ = conv_backward(ssd, cuda, xs, k, dys, bias=False, with_dx=False)
    assert same_bits(tk.grad.cpu().numpy(), dw) and np.abs(dw).max() > 0
    # a single tensor, only the kernel requiring a gradient: the same entry point without dx
    t0, tk2 = _dev(cuda, xs[0]), _dev(cuda, k).requires_grad_()
    ssd.pointwise_conv(t0, tk2).backward(_dev(cuda, dys[0]))
    _, dw0, _ = conv_backward(ssd, cuda, xs[:1], k, dys[:1], bias=False, with_dx=False)
    assert t0.grad is None and same_bits(tk2.grad.cpu().numpy(), dw0)


# ----------------------------------------------------------------------------- 5. the batch norm with ReLU6
def _same_bits_or_nan(a, b):
    """Bit equality where either is a number; a NaN only has to meet a NaN (its payload is not pinned)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and same_bits(np.where(na, f32(0), a), np.where(nb, f32(0), b))


def _bn_inputs(rng, rows, C):
    xs = [rng.normal(0.3, 1.5, (r, C)).astype(f32) for r in rows]
    dys = [rng.normal(0, 1, (r, C)).astype(f32) for r in rows]
    gammas = [rng.uniform(2.0, 4.0, C).astype(f32) for _ in rows]         # y = gamma * xhat + beta: a few percent beyond 6
    betas = [rng.normal(0, 0.3, C).astype(f32) for _ in rows]
    mms = [rng.normal(0, 0.1, C).astype(f32) for _ in rows]
    mvs = [rng.uniform(0.5, 1.5, C).astype(f32) for _ in rows]
    return xs, gammas, betas, mms, mvs, dys


@pytest.mark.parametrize("C", [6, 32, 1024])
def test_batch_norm_relu6_is_the_headers_float32_sequence_bit_for_bit(ssd, cuda, C):
    """out and dx against the header's float32 sequence in numpy on the kernel's own statistics and its own dgamma / dbeta (the
    method of test_gpu_head_train_edges.py).  Channel 0's beta is chosen so that one y is exactly 0, channel 1's so that one y is
    exactly 6 (the statistics do not depend on beta: a first call gives them); channel 2 holds a NaN, which makes every y of that
    channel NaN: out 0, gate closed."""
    rows = [300, 37]
    xs, gammas, betas, mms, mvs, dys = _bn_inputs(np.random.default_rng(C), rows, C)
    for x in xs:
        x[3, 2] = np.nan
    first = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, act="relu6")
    for i, g in enumerate(first):
        assert same_bits(g["invstd"][[0, 1]], href.invstd_f32(g["var"])[[0, 1]])
        t = ((xs[i] - g["mean"]) * (gammas[i] * g["invstd"])).astype(f32)
        betas[i][0] = -t[5, 0]                                            # t + (-t) = 0
        cand = (6 - t[:, 1]).astype(f32)
        hit = np.nonzero((t[:, 1] + cand).astype(f32) == f32(6))[0]
        assert hit.size
        betas[i][1] = cand[hit[0]]
    got = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys, act="relu6")
    again = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys, act="relu6")
    for i, g in enumerate(got):
        for name in ("mean", "var", "invstd"):
            assert same_bits(np.delete(g[name], 2), np.delete(first[i][name], 2)) and np.isnan(g[name][2])
        ypre, out, dx = ref.bn_act_f32(xs[i], gammas[i], betas[i], g["mean"], None, "relu6", dys[i], dgamma=g["dgamma"], dbeta=g["dbeta"],
                                       invstd=g["invstd"])
        assert (ypre == 0).any() and (ypre == 6).any() and np.isnan(ypre).any()
        opened = ref.gate_f32(ypre, "relu6")
        with np.errstate(invalid="ignore"):
            assert opened.any() and (ypre[:, 3:] <= 0).any() and (ypre[:, 3:] >= 6).any()      # both gates occur, and the open middle
        assert same_bits(g["y"], out), i
        assert np.all(g["y"][:, 2] == 0) and g["dbeta"][2] == 0              # a NaN y: out 0, gate closed
        assert np.all(g["y"][ypre == 6] == 6) and np.all(g["y"][ypre == 0] == 0)
        assert _same_bits_or_nan(g["dx"], dx), i
        # dgamma / dbeta of the finite channels: the double sums of the gated terms, rounded once
        keep = np.setdiff1d(np.arange(C), [2])
        gate = np.where(opened, dys[i], f32(0))[:, keep].astype(f64)
        xhat = ((xs[i] - g["mean"]) * g["invstd"]).astype(f32)[:, keep].astype(f64)
        for name, terms in (("dbeta", gate), ("dgamma", gate * xhat)):
            want, tol = href.double_sum_bound(terms)
            assert np.all(np.abs(g[name][keep].astype(f64) - want.astype(f64)) <= tol), (i, name)
        for name in g:
            assert _same_bits_or_nan(g[name], again[i][name]), (i, name)


@pytest.mark.parametrize("C", [6, 256])
def test_batch_norm_relu_through_the_new_entry_points_is_the_old_pair_bit_for_bit(ssd, cuda, C):
    rows = [442, 35, 1]
    xs, gammas, betas, mms, mvs, dys = _bn_inputs(np.random.default_rng(C + 2), rows, C)
    old = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)
    new = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys, act="relu")
    six = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys, act="relu6")
    for i in range(len(rows)):
        for name in old[i]:
            assert same_bits(old[i][name], new[i][name]), (i, name)
        assert np.isfinite(old[i]["dx"]).all()
    assert old[0]["y"].max() > 6 and six[0]["y"].max() == 6 and not same_bits(old[0]["dx"], six[0]["dx"])


@pytest.mark.parametrize("C", [6, 256])
def test_batch_norm_relu6_inference_form_is_the_oracles_epilogue(ssd, cuda, oracle_ops, C):
    rows = [442, 35, 1]
    xs, gammas, betas, mms, mvs, _ = _bn_inputs(np.random.default_rng(C + 3), rows, C)
    got = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, training=0, act="relu6")
    for i, g in enumerate(got):
        want = oracle_ops.bn_act(xs[i], gammas[i], betas[i], mms[i], mvs[i], "relu6")
        assert same_bits(g["y"], want)
        if i == 0:
            assert want.max() == 6 and want.min() == 0 and ((want > 0) & (want < 6)).any()
        assert same_bits(g["mm"], mms[i]) and same_bits(g["mv"], mvs[i]) and np.isnan(g["mean"]).all()
        ty = ssd.batch_norm_act(_dev(cuda, xs[i]), *[_dev(cuda, v) for v in (gammas[i], betas[i], mms[i], mvs[i])], training=False)
        assert same_bits(ty.cpu().numpy(), want)


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_come_before_any_launch(ssd, cuda):
    L = ssd.lib()
    H, W, C = 6, 8, 8
    full = lambda shape: cuda.full(shape, 7.0, device="cuda")
    x, w = cuda.zeros((B, H, W, C), device="cuda"), cuda.zeros((3, 3, C, 1), device="cuda")
    dy1, out, dx, dw = cuda.zeros((B, H, W, C), device="cuda"), full((B, H, W, C)), full((B, H, W, C)), full((3, 3, C, 1))
    ws = cuda.empty(1 << 20, dtype=cuda.uint8, device="cuda")
    s = ssd.train_calls.stream(x.device)

    def fwd(c=C, stride=1, h=H, ww=W, xp=x.data_ptr()):
        return L.ssd_depthwise_train_forward(xp, B, h, ww, c, w.data_ptr(), stride, out.data_ptr(), s)

    def bwd(c=C, stride=1, h=H, ww=W, dyp=dy1.data_ptr(), wsb=ws.numel()):
        return L.ssd_depthwise_train_backward(x.data_ptr(), dyp, B, h, ww, c, w.data_ptr(), stride, dx.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, s)
    need = L.ssd_depthwise_train_workspace_bytes(B, H, W, C, 1)
    assert 0 < need <= ws.numel()
    for what, rcs, sized in (("C = 6", (fwd(c=6), bwd(c=6)), L.ssd_depthwise_train_workspace_bytes(B, H, W, 6, 1)),
                             ("stride 3", (fwd(stride=3), bwd(stride=3)), L.ssd_depthwise_train_workspace_bytes(B, H, W, C, 3)),
                             ("stride 2 on 5 x 8", (fwd(stride=2, h=5), bwd(stride=2, h=5)), L.ssd_depthwise_train_workspace_bytes(B, 5, W, C, 2)),
                             ("C = 1028 backward", (bwd(c=1028),), L.ssd_depthwise_train_workspace_bytes(B, H, W, 1028, 1))):
        assert all(rc == -1 for rc in rcs) and sized == 0, what
    assert bwd(stride=2, h=5) == -1 and b"parity" in L.ssd_last_error()
    assert bwd(wsb=need - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    assert fwd(xp=x.data_ptr() + 4) == -1 and bwd(dyp=dy1.data_ptr() + 4) == -1 and b"16-byte" in L.ssd_last_error()
    # the batch norm: act = 0 (and 3) through both calls
    Lv = ssd._lib.SsdBnLevel
    vec = [cuda.zeros(C, device="cuda") for _ in range(9)]
    x2, y2 = x.view(-1, C), out.view(-1, C)
    lv = (Lv * 1)(Lv(x2.shape[0], x2.data_ptr(), x2.data_ptr(), y2.data_ptr(), *[v.data_ptr() for v in vec]))
    for act in (0, 3):
        assert L.ssd_bn_act_train_forward(lv, 1, C, act, 1, 1e-3, 0.007, ws.data_ptr(), ws.numel(), s) == -1 and b"act" in L.ssd_last_error()
        assert L.ssd_bn_act_train_backward(lv, 1, C, act, ws.data_ptr(), ws.numel(), s) == -1 and b"act" in L.ssd_last_error()
    # the 1x1 backward: a short workspace, a misaligned dx
    CL = ssd._lib.SsdConvLevel
    Cout = 16
    dyc, wc, dwc = cuda.zeros((B, H, W, Cout), device="cuda"), cuda.zeros((1, 1, C, Cout), device="cuda"), full((1, 1, C, Cout))
    clv = lambda o: (CL * 1)(CL(H, W, x.data_ptr(), dyc.data_ptr(), o))
    pneed = L.ssd_pointwise_train_workspace_bytes(clv(dx.data_ptr()), 1, B, C, Cout)
    assert 0 < pneed <= ws.numel() and L.ssd_pointwise_train_workspace_bytes(clv(dx.data_ptr()), 1, B, 6, Cout) == 0
    pw = lambda o, wsb: L.ssd_pointwise_train_backward(clv(o), 1, B, C, Cout, wc.data_ptr(), dwc.data_ptr(), ws.data_ptr(), wsb, s)
    assert pw(dx.data_ptr(), pneed - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    assert pw(dx.data_ptr() + 4, ws.numel()) == -1
    # ssd_conv_train_backward keeps refusing the data gradient of a 1x1 convolution, and conv_same keeps raising
    assert L.ssd_conv_train_backward(clv(dx.data_ptr()), 1, B, C, Cout, 1, 1, wc.data_ptr(), dwc.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == -1
    assert b"1x1" in L.ssd_last_error()
    cuda.cuda.synchronize()
    for t in (out, dx, dw, dwc):                                        # nothing ran
        assert bool((t == 7.0).all())
    tx = cuda.zeros((B, H, W, C), device="cuda", requires_grad=True)
    y = ssd.conv_same(tx, wc.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="1x1"):
        y.backward(dyc)
    assert fwd() == 0 and bwd(wsb=need) == 0 and pw(dx.data_ptr(), pneed) == 0       # and the same calls with good arguments run
    cuda.cuda.synchronize()
    assert bool((out == 0).all()) and bool((dw == 0).all()) and bool((dx == 0).all()) and bool((dwc == 0).all())


# ----------------------------------------------------------------------------- 7. inference mode
def _engine(ssd, cuda, seed, keep=()):
    W = ssd.synthetic_weights(TINY_PARAMS, seed=seed, logits_bias=-4.0)
    img = np.random.default_rng(seed + 1).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    eng = ssd.Engine(TINY_PARAMS, W, device=0)
    eng.forward(cuda.from_numpy(img).cuda())
    kept = {k: eng.get_tensor(k) for k in ("c3", "c4", "c5") + tuple(keep)}
    eng.close()
    return W, img, kept


def test_trainable_mobilenet_in_inference_mode_is_the_engine_bit_for_bit(ssd, cuda):
    W, img, kept = _engine(ssd, cuda, 31)
    m = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", keep_features=True).eval()
    with cuda.no_grad():
        cs = m(cuda.from_numpy(img).cuda())
    assert [tuple(c.shape[1:]) for c in cs] == [(16, 16, 256), (8, 8, 512), (4, 4, 1024)]
    for name, c in zip(("c3", "c4", "c5"), cs):
        assert np.array_equal(c.cpu().numpy(), kept[name]) and np.abs(kept[name]).max() > 0, name
    assert len(m.features) == 26 and cuda.equal(m.features["Conv2d_13_pointwise"], cs[2])
    for k, v in m.statistics().items():                                 # inference mode moves nothing
        assert same_bits(v.cpu().numpy(), W[k]), k


# ----------------------------------------------------------------------------- 8. training mode
def test_trainable_mobilenet_in_training_mode_against_the_float64_restatement(ssd, cuda):
    """Conv2d_1 .. 13 on batch statistics from Conv2d_0's output: c3, c4, c5, the gradient of sum(c_l * d_l) (d_l random, both signs)
    with respect to all 78 variables, and the 52 moving statistics, per tensor and norm-wise (head_train_ref.rel) against a float64
    CPU torch restatement.  A ReLU6 gate that flips between two precisions moves the lower layers' gradients by 1e-2 of their
    maximum, so the restatement takes its gates from the run under test (layer by layer out = y * open + 6 * hi, open and hi read
    from the module's features); the gates themselves are pinned by the bit-for-bit batch-norm test above.  Bound: the kernels'
    figure may be at most FACTOR = 4 x the figure of a float32 CPU torch run with the same forced gates, the project's margin for
    the same quantities in the head and FPN tests.  Measured on an MI355X (profiles/r19_backbone_train.log): gates 1 521 159 open, 118
    at 6, 1 509 763 closed; the worst ratios are 2.13 x (d Conv2d_7_pointwise/BatchNorm/gamma: 9.61e-6 against 4.52e-6) and 2.03 x (d
    Conv2d_9_pointwise/BatchNorm/gamma: 1.14e-5 against 5.59e-6); c3, c4, c5 and the moving statistics stay below 1.7 x."""
    import torch
    FACTOR = 4.0
    W = ssd.synthetic_weights(TINY_PARAMS, seed=41, logits_bias=-4.0)
    img = np.random.default_rng(42).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    m = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", keep_features=True).train()
    x0 = m.first_conv(cuda.from_numpy(img).cuda())
    rng = np.random.default_rng(43)
    ds = [rng.normal(0, 1, (B, h, h, c)).astype(f32) for h, c in ((16, 256), (8, 512), (4, 1024))]
    cs = m.body(x0)
    cuda.autograd.backward(cs, [_dev(cuda, d) for d in ds])
    feats = {k: v.cpu().numpy() for k, v in m.features.items()}
    gates = ref.gates_of(feats)
    kinds = [sum(int(g[0].sum()) for g in gates.values()), sum(int(g[1].sum()) for g in gates.values()),
             sum(int((~g[0] & ~g[1]).sum()) for g in gates.values())]
    print("mobilenet train mode gates: open %d, at 6 %d, closed %d" % tuple(kinds))
    assert len(gates) == 26 and all(kinds)                              # gates of all three kinds occur
    runs = {}
    for dtype in (torch.float64, torch.float32):
        outs, T, S = ref.torch_mobilenet(W, x0.cpu().numpy(), dtype, gates)
        torch.autograd.backward(outs, [torch.tensor(d.astype(f64), dtype=dtype) for d in ds])
        rows = [("c%d" % (3 + l), outs[l].detach().numpy()) for l in range(3)]
        rows += [("d " + k, v.grad.numpy()) for k, v in T.items()] + [(k, v.numpy()) for k, v in S.items()]
        runs[dtype] = dict(rows)
    got = {"c%d" % (3 + l): cs[l].detach().cpu().numpy() for l in range(3)}
    got.update({"d " + k: v.grad.cpu().numpy() for k, v in m.named_variables().items()})
    got.update({k: v.cpu().numpy() for k, v in m.statistics().items()})
    assert set(got) == set(runs[torch.float64]) and len(got) == 3 + 78 + 52
    bad, worst = [], (0.0, None)
    for name, r64 in runs[torch.float64].items():
        assert np.abs(r64).max() > 0, name                              # no vacuous comparison
        yard, d = ref.rel(runs[torch.float32][name], r64), ref.rel(got[name], r64)
        print("mobilenet train mode %-56s float32 torch %.3g  kernels %.3g  ratio %.2f" % (name, yard, d, d / yard))
        worst = max(worst, (d / yard, name))
        if not d <= FACTOR * yard:
            bad.append((name, d, yard))
    print("mobilenet train mode worst ratio %.2f (%s)" % worst)
    assert not bad, bad
    for k, v in m.statistics().items():
        assert not np.array_equal(v.cpu().numpy(), W[k]), k


# ----------------------------------------------------------------------------- 9. the bridge through the FPN
def test_fpn_gives_the_gradients_of_c3_c4_c5_against_the_float64_restatement(ssd, cuda):
    """d c3, d c4, d c5 of sum(p_l * d_l) from TrainableFPN on features that require a gradient, against fpn() in float64 CPU torch
    with its inputs as leaves; yardstick the float32 run of the same graph, FACTOR = 4 (the FPN training test's bound).  Measured on
    an MI355X (profiles/r19_backbone_train.log): 1.54 x, 1.45 x and 1.02 x (d c3: 9.96e-7 against 6.46e-7)."""
    import torch
    FACTOR = 4.0
    W, _, kept = _engine(ssd, cuda, 13)
    cs = [kept["c3"], kept["c4"], kept["c5"]]
    rng = np.random.default_rng(14)
    ds = [rng.normal(0, 1, (B, h, w, 256)).astype(f32) for h, w in [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]]
    runs = {}
    for dtype in (torch.float64, torch.float32):
        outs, leaves = ref.torch_fpn_inputs(W, cs, dtype)
        torch.autograd.backward(outs, [torch.tensor(d.astype(f64), dtype=dtype) for d in ds])
        runs[dtype] = [t.grad.numpy() for t in leaves]
    m = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
    tc = [_dev(cuda, c).requires_grad_() for c in cs]
    cuda.autograd.backward(m(tc), [_dev(cuda, d) for d in ds])
    bad = []
    for l in range(3):
        r64 = runs[torch.float64][l]
        assert np.abs(r64).max() > 0
        yard, d = ref.rel(runs[torch.float32][l], r64), ref.rel(tc[l].grad.cpu().numpy(), r64)
        print("fpn bridge d c%d  float32 torch %.3g  kernels %.3g  ratio %.2f" % (3 + l, yard, d, d / yard))
        if not d <= FACTOR * yard:
            bad.append((l, d, yard))
    assert not bad, bad
    # only c4 requiring a gradient: it gets the same bits, the others none
    m2 = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
    t2 = [_dev(cuda, cs[0]), _dev(cuda, cs[1]).requires_grad_(), _dev(cuda, cs[2])]
    cuda.autograd.backward(m2(t2), [_dev(cuda, d) for d in ds])
    assert t2[0].grad is None and t2[2].grad is None and same_bits(t2[1].grad.cpu().numpy(), tc[1].grad.cpu().numpy())
    for k, v in m.named_variables().items():                            # and the variables' gradients do not depend on the bridge
        assert same_bits(v.grad.cpu().numpy(), m2.named_variables()[k].grad.cpu().numpy()), k


def test_fpn_on_features_without_a_gradient_runs_the_frozen_backbone_sequence(ssd, cuda, monkeypatch):
    """Outputs and every variable's gradient have the bits of a second run, of a run whose features require a gradient, and the
    launch sequence is the frozen-backbone one: eight ssd_conv_train_backward calls, no ssd_pointwise_train_backward."""
    W, _, kept = _engine(ssd, cuda, 15)
    cs = [kept["c3"], kept["c4"], kept["c5"]]
    rng = np.random.default_rng(16)
    ds = [_dev(cuda, rng.normal(0, 1, (B, h, w, 256)).astype(f32)) for h, w in [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]]
    fpn_train = ssd.fpn_train
    calls = []
    real_conv = fpn_train._conv_backward

    def conv(xs, kernel, dys, stride, want_dx, want_dbias=False, entry="conv"):
        calls.append("pointwise" if entry == "pointwise" else (kernel.shape[0], stride, bool(want_dx)))
        return real_conv(xs, kernel, dys, stride, want_dx, want_dbias, entry)
    monkeypatch.setattr(fpn_train, "_conv_backward", conv)
    runs = []
    for grad in (False, False, True):
        del calls[:]
        m = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
        ps = m([_dev(cuda, c).requires_grad_(grad) for c in cs])
        cuda.autograd.backward(ps, ds)
        runs.append(([p.detach().cpu().numpy() for p in ps], {k: v.grad.cpu().numpy() for k, v in m.named_variables().items()}, list(calls)))
    today = [(3, 2, True), (3, 2, False), (3, 1, True), (1, 1, False), (3, 1, True), (1, 1, False), (3, 1, True), (1, 1, False)]
    assert runs[0][2] == today and runs[1][2] == today
    assert runs[2][2] == [(3, 2, True), (3, 2, True), (3, 1, True), "pointwise", (3, 1, True), "pointwise", (3, 1, True), "pointwise"]
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert same_bits(a, b)
        assert len(other[1]) == 18
        for k, v in runs[0][1].items():
            assert same_bits(v, other[1][k]) and np.abs(v).max() > 0, k


# ----------------------------------------------------------------------------- 10. the loop
def test_the_loop_closes_through_a_checkpoint(ssd, cuda, tmp_path):
    """images -> TrainableMobileNet -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward -> one TrainStep over
    the three modules' variables with Conv2d_0 frozen -> save -> a fresh Detector on that checkpoint."""
    loop_closes_through_a_checkpoint(ssd, cuda, tmp_path, ssd.TrainableMobileNet, TINY_PARAMS, "MobilenetV1/Conv2d_0/", lambda variables: set(),
                                     "c5")
