"""The TRAIN FPN on the GPU (include/ssd_hip.h, "the TRAIN FPN"): the generalised convolution's forward against ssd_conv2d and its
stride-2 data gradient against the CPU oracle bit for bit, the weight gradient exactly on integers and within the order-free fp32
bound on random data, ssd_fpn_merge_backward against the header's line, the refusals, TrainableFPN in inference mode against the
engine bit for bit and in training mode against a float64 restatement, and the closed loop through a checkpoint."""
import ctypes

import numpy as np
import pytest

from helpers import fpn_train_ref as ref
from helpers import head_train_ref as href
from helpers.head_train_gpu import conv_backward, conv_backward_raw, conv_forward_raw, dev as _dev, same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 2
LP = {"gamma": 2.0, "alpha": 0.25}
S2_SIZES = [(6, 8), (5, 7)]                                           # 5 x 7 -> 3 x 4: the odd case of conv2d_same's explicit pad
S2_WIDTHS = [(256, 256), (40, 24)]


def _data(rng, shape, integers=False, scale=1.0):
    return rng.integers(-3, 4, shape).astype(f32) if integers else rng.normal(0, scale, shape).astype(f32)


def _kernel(rng, k, Cin, Cout, integers=False):
    return rng.integers(-2, 3, (k, k, Cin, Cout)).astype(f32) if integers else rng.normal(0, 0.05, (k, k, Cin, Cout)).astype(f32)


# ----------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("Cin,Cout", [(8, 256), (116, 256), (1024, 32)])
def test_forward_1x1_is_ssd_conv2d_bit_for_bit(ssd, cuda, Cin, Cout):
    rng = np.random.default_rng(Cin + Cout)
    xs = [_data(rng, (B, h, w, Cin)) for h, w in ((5, 7), (3, 4))]
    w = _kernel(rng, 1, Cin, Cout)
    ys = ssd.conv_same([_dev(cuda, x) for x in xs], _dev(cuda, w))
    for x, y in zip(xs, ys):
        want = ssd.ssd.conv2d(_dev(cuda, x), w)
        assert y.shape == want.shape and cuda.equal(y, want), x.shape


@pytest.mark.parametrize("Cin,Cout", S2_WIDTHS)
def test_forward_stride_2_is_ssd_conv2d_bit_for_bit(ssd, cuda, Cin, Cout):
    rng = np.random.default_rng(Cin * 2 + Cout)
    xs = [_data(rng, (B, h, w, Cin)) for h, w in S2_SIZES]
    w = _kernel(rng, 3, Cin, Cout)
    ys = ssd.conv_same([_dev(cuda, x) for x in xs], _dev(cuda, w), stride=2)
    for x, y in zip(xs, ys):
        want = ssd.ssd.conv2d(_dev(cuda, x), w, stride=2, mode="EXPLICIT")
        assert tuple(y.shape[1:3]) == ref.out_hw(x.shape[1], x.shape[2], 2)
        assert y.shape == want.shape and cuda.equal(y, want), x.shape


def test_forward_1x1_with_the_upsampled_operand_is_ssd_conv2d_bit_for_bit(ssd, cuda):
    rng = np.random.default_rng(46)
    Cin, Cout = 116, 256
    x, up, w = _data(rng, (B, 4, 6, Cin)), _data(rng, (B, 2, 3, Cout)), _kernel(rng, 1, Cin, Cout)
    y = ssd.conv_same(_dev(cuda, x), _dev(cuda, w), up=_dev(cuda, up))
    want = ssd.ssd.conv2d(_dev(cuda, x), w, up=_dev(cuda, up))
    assert cuda.equal(y, want)
    assert not cuda.equal(y, ssd.ssd.conv2d(_dev(cuda, x), w))
    # two levels, each with its own operand
    x2, up2 = _data(rng, (B, 2, 2, Cin)), _data(rng, (B, 1, 1, Cout))
    ys = ssd.conv_same([_dev(cuda, x), _dev(cuda, x2)], _dev(cuda, w), up=[_dev(cuda, up), _dev(cuda, up2)])
    assert cuda.equal(ys[0], want) and cuda.equal(ys[1], ssd.ssd.conv2d(_dev(cuda, x2), w, up=_dev(cuda, up2)))


# ----------------------------------------------------------------------------- 2. the stride-2 data gradient
@pytest.mark.parametrize("Cin,Cout", S2_WIDTHS)
def test_stride_2_data_gradient_is_the_oracles_convolution_of_the_dilated_gradient(ssd, cuda, oracle_ops, Cin, Cout):
    """dx = conv2d(D, w'), D the zero-dilated dy: bit for bit.  1 x 1 and 2 x 2 -> 1 x 1 are the p7 of a 128-pixel image."""
    rng = np.random.default_rng(Cin * 3 + Cout)
    sizes = S2_SIZES + [(1, 1), (2, 2)]
    xs = [_data(rng, (B, h, w, Cin)) for h, w in sizes]
    dys = [_data(rng, (B,) + ref.out_hw(h, w, 2) + (Cout,)) for h, w in sizes]
    w = _kernel(rng, 3, Cin, Cout)
    dxs, _, _ = conv_backward(ssd, cuda, xs, w, dys, stride=2, bias=False)
    wr = href.rotated_transposed(w)
    for (h, ww), dy, dx in zip(sizes, dys, dxs):
        want = oracle_ops.conv2d(ref.dilate(dy, h, ww), wr)
        assert dx.shape == want.shape and np.array_equal(dx, want), (h, ww)
        assert np.abs(dx).max() > 0


# ----------------------------------------------------------------------------- 3. the weight gradient on integers
def _exact_case(ssd, cuda, sizes, k, stride, Cin, Cout, seed):
    rng = np.random.default_rng(seed)
    xs = [_data(rng, (B, h, w, Cin), True) for h, w in sizes]
    dys = [_data(rng, (B,) + ref.out_hw(h, w, stride) + (Cout,), True) for h, w in sizes]
    w = _kernel(rng, k, Cin, Cout, True)
    dw64, _, absmax, _ = ref.integer_premise(xs, w, dys, stride)
    assert absmax < 2 ** 24 and np.abs(dw64).max() > 0                # the premise, checked
    _, dw, _ = conv_backward(ssd, cuda, xs, w, dys, stride=stride, bias=False, with_dx=False)
    assert dw.shape == w.shape and np.array_equal(dw.astype(np.float64), dw64)


@pytest.mark.parametrize("Cout", [24, 256])
@pytest.mark.parametrize("Cin", [8, 116, 132, 1024])
def test_weight_gradient_1x1_is_exact_on_small_integers(ssd, cuda, Cin, Cout):
    """116 and 132 are multiples of 4 and not of 8 (ShuffleNet's c3 has 116); 132 and 1024 take more than one 128-channel tile,
    132 with 4 channels in the last.  13 x 17 x 2 = 442 rows: no multiple of the K-step, two slices of 256."""
    _exact_case(ssd, cuda, [(13, 17)], 1, 1, Cin, Cout, Cin + Cout)


@pytest.mark.parametrize("Cin,Cout", S2_WIDTHS)
def test_weight_gradient_stride_2_is_exact_on_small_integers(ssd, cuda, Cin, Cout):
    _exact_case(ssd, cuda, S2_SIZES + [(1, 1), (2, 2), (13, 17)], 3, 2, Cin, Cout, Cin * 5 + Cout)


def test_weight_gradient_is_exact_over_several_slices_and_two_levels(ssd, cuda):
    """1x1, 8 -> 24: one tile, slices of 256 output rows: 40 x 28 x 2 = 2240 rows are 8 full slices and one of 192, the second
    level (442 rows) two more.  Stride 2, 40 -> 24 over 39 x 55 (20 x 28 x 2 = 1120 output rows, 5 slices) and 13 x 17."""
    assert ref.rows_per_slice([2240, 442], 8, 24, 1) == 256 and ref.rows_per_slice([1120, 126], 40, 24, 3) == 256
    _exact_case(ssd, cuda, [(40, 28), (13, 17)], 1, 1, 8, 24, 7)
    _exact_case(ssd, cuda, [(39, 55), (13, 17)], 3, 2, 40, 24, 8)


def test_3x3_stride_1_through_the_new_entry_point_is_the_old_one_bit_for_bit(ssd, cuda):
    """ssd_conv3x3_train_* and ssd_conv_train_* with k = 3, stride = 1, up = NULL, both straight through the C ABI: the same
    workspace size and the same bits in the outputs, dx, dw and dbias; conv3x3_same through autograd gives those bits too."""
    rng = np.random.default_rng(9)
    sizes, Cin, Cout = [(13, 17), (4, 5)], 64, 40
    xs = [_data(rng, (B, h, w, Cin)) for h, w in sizes]
    dys = [_data(rng, (B, h, w, Cout)) for h, w in sizes]
    w, bias = _kernel(rng, 3, Cin, Cout), _data(rng, (Cout,), scale=0.1)
    ys_old, need_old = conv_forward_raw(ssd, cuda, xs, w, bias)
    ys_new, need_new = conv_forward_raw(ssd, cuda, xs, w, bias, general=True)
    dxs_old, dw_old, db_old = conv_backward_raw(ssd, cuda, xs, w, dys, True, True)
    dxs_new, dw_new, db_new = conv_backward_raw(ssd, cuda, xs, w, dys, True, True, general=True)
    assert need_old == need_new
    tx = [_dev(cuda, x).requires_grad_() for x in xs]
    tw, tb = _dev(cuda, w).requires_grad_(), _dev(cuda, bias).requires_grad_()
    ys = ssd.conv3x3_same(tx, tw, tb)
    cuda.autograd.backward(ys, [_dev(cuda, d) for d in dys])
    for old, new, got in zip(ys_old + dxs_old, ys_new + dxs_new, [y.detach() for y in ys] + [t.grad for t in tx]):
        assert np.isfinite(old).all() and same_bits(old, new) and same_bits(old, got.cpu().numpy())
    assert same_bits(dw_old, dw_new) and same_bits(dw_old, tw.grad.cpu().numpy()) and np.abs(dw_old).max() > 0
    assert same_bits(db_old, db_new) and same_bits(db_old[:Cout], tb.grad.cpu().numpy()) and np.abs(db_old).max() > 0


def test_partial_needs_give_the_bits_of_a_zero_gradient(ssd, cuda):
    """Only level 0's output is differentiated and only x0 requires a gradient: x1 gets none, and x0.grad and dw have the bits of a
    run where both outputs are used and level 1's dy is all zeros."""
    rng = np.random.default_rng(21)
    sizes, Cin, Cout = [(4, 6), (2, 2)], 8, 16
    xs = [_data(rng, (B, h, w, Cin)) for h, w in sizes]
    w, dy0 = _kernel(rng, 3, Cin, Cout), _data(rng, (B, 4, 6, Cout))
    x0, x1, tw = _dev(cuda, xs[0]).requires_grad_(), _dev(cuda, xs[1]), _dev(cuda, w).requires_grad_()
    ys = ssd.conv_same([x0, x1], tw)
    (ys[0] * _dev(cuda, dy0)).sum().backward()
    assert x1.grad is None
    dxs, dw, _ = conv_backward(ssd, cuda, xs, w, [dy0, np.zeros((B, 2, 2, Cout), f32)], bias=False)
    assert same_bits(x0.grad.cpu().numpy(), dxs[0]) and same_bits(tw.grad.cpu().numpy(), dw) and np.abs(dw).max() > 0


def test_up_with_a_gradient_and_features_without(ssd, cuda):
    """1x1 with `up`, two levels, only up[0] requiring a gradient: it is fpn_merge_backward(dy0), up[1] gets none and nothing
    raises; once a feature requires a gradient the backward raises the 1x1 RuntimeError."""
    rng = np.random.default_rng(46)
    Cin, Cout = 116, 256
    xs = [_dev(cuda, _data(rng, (B, 4, 6, Cin))), _dev(cuda, _data(rng, (B, 2, 2, Cin)))]
    ups = [_dev(cuda, _data(rng, (B, 2, 3, Cout))).requires_grad_(), _dev(cuda, _data(rng, (B, 1, 1, Cout)))]
    w = _dev(cuda, _kernel(rng, 1, Cin, Cout))
    dys = [_dev(cuda, _data(rng, (B, 4, 6, Cout))), _dev(cuda, _data(rng, (B, 2, 2, Cout)))]
    cuda.autograd.backward(ssd.conv_same(xs, w, up=ups), dys)
    assert ups[1].grad is None and float(ups[0].grad.abs().max()) > 0
    assert same_bits(ups[0].grad.cpu().numpy(), ssd.fpn_merge_backward(dys[0]).cpu().numpy())
    xs[0].requires_grad_()
    ys = ssd.conv_same(xs, w, up=ups)
    with pytest.raises(RuntimeError, match="1x1"):
        cuda.autograd.backward(ys, dys)


# ----------------------------------------------------------------------------- 4. the weight gradient on random data
@pytest.mark.parametrize("k,stride,Cin,Cout", [(1, 1, 116, 256), (1, 1, 1024, 24), (3, 2, 256, 256), (3, 2, 40, 24)])
def test_weight_gradient_obeys_the_order_free_fp32_bound(ssd, cuda, k, stride, Cin, Cout):
    """|dw - dw64| <= gamma_n * sum |x * dy| per element, n = the element's number of products (output positions whose tap lies
    inside the input), gamma_n = n u / (1 - n u), u = 2^-24: head_train_ref.wgrad_bound's derivation, the bound of ANY order."""
    rng = np.random.default_rng(k * 1000 + Cin + Cout)
    sizes = [(13, 17), (5, 7)]
    xs = [_data(rng, (B, h, w, Cin)) for h, w in sizes]
    dys = [_data(rng, (B,) + ref.out_hw(h, w, stride) + (Cout,)) for h, w in sizes]
    w = _kernel(rng, k, Cin, Cout)
    dw64, bound, absum = ref.wgrad_bound(xs, w, dys, stride)
    _, dw, _ = conv_backward(ssd, cuda, xs, w, dys, stride=stride, bias=False, with_dx=False)
    err = np.abs(dw.astype(np.float64) - dw64)
    print("fpn wgrad k=%d s=%d %d->%d: max |dw - dw64| / sum|x dy| = %.3g" % (k, stride, Cin, Cout, (err / absum).max()))
    assert np.isfinite(dw).all() and np.all(err <= bound) and np.abs(dw64).max() > 0
    _, dw2, _ = conv_backward(ssd, cuda, xs, w, dys, stride=stride, bias=False, with_dx=False)
    assert same_bits(dw, dw2)


# ----------------------------------------------------------------------------- 5. the merge
@pytest.mark.parametrize("C", [6, 256])
def test_merge_backward_is_the_headers_line_bit_for_bit(ssd, cuda, C):
    rng = np.random.default_rng(C)
    H, W = 3, 5
    g, gs, base = _data(rng, (B, 2 * H, 2 * W, C)), _data(rng, (B, H, W, C)), _data(rng, (B, H, W, C))
    gate = _data(rng, (B, H, W, C))
    gate.reshape(-1)[:6] = [-0.0, 0.0, np.nan, 1.0, -1.0, np.inf]
    g.reshape(-1)[0] = np.nan                                           # behind a closed gate: must not spread
    assert np.isnan(gate).any() and (gate > 0).any() and (gate <= 0).any()
    for use_base in (False, True):
        for use_gate in (False, True):
            for same in (False, True):
                src = gs if same else g
                got = ssd.fpn_merge_backward(_dev(cuda, src), _dev(cuda, base) if use_base else None,
                                             _dev(cuda, gate) if use_gate else None, same_size=same).cpu().numpy()
                want = ref.merge_f32(src, base if use_base else None, gate if use_gate else None, same)
                assert same_bits(got, want), (use_base, use_gate, same)
                if use_gate and not same:
                    assert np.isfinite(got.reshape(-1)[0])
    tb = _dev(cuda, base)                                               # in place: out is base
    ssd.fpn_merge_backward(_dev(cuda, g), tb, out=tb)
    assert same_bits(tb.cpu().numpy(), ref.merge_f32(g, base))


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_come_before_any_launch(ssd, cuda):
    L, Lv = ssd.lib(), ssd._lib.SsdConvLevel
    H, W, Cin, Cout = 4, 6, 8, 16
    x, dy, out = cuda.zeros((B, H, W, Cin), device="cuda"), cuda.zeros((B, H, W, Cout), device="cuda"), cuda.full((B, H, W, Cout), 7.0, device="cuda")
    dx, up = cuda.full((B, H, W, Cin), 7.0, device="cuda"), cuda.zeros((B, H // 2, W // 2, Cout), device="cuda")
    w, dw = cuda.zeros((3, 3, Cin, Cout), device="cuda"), cuda.full((3, 3, Cin, Cout), 7.0, device="cuda")
    ws = cuda.empty(1 << 22, dtype=cuda.uint8, device="cuda")
    s = ctypes.c_void_p(cuda.cuda.current_stream().cuda_stream)
    ups = (ctypes.c_void_p * 1)(up.data_ptr())

    def lv(h=H, ww=W, o=out):
        return (Lv * 1)(Lv(h, ww, x.data_ptr(), dy.data_ptr(), o.data_ptr() if o is not None else None))

    def fwd(k=3, stride=1, cin=Cin, levels=None, up_=None, wsb=ws.numel()):
        return L.ssd_conv_train_forward(levels or lv(), 1, B, cin, Cout, k, stride, w.data_ptr(), None, up_, ws.data_ptr(), wsb, s)

    def bwd(k=3, stride=1, cin=Cin, o=None, wsb=ws.numel()):
        return L.ssd_conv_train_backward(lv(o=o), 1, B, cin, Cout, k, stride, w.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), wsb, s)
    need = L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 3, 1, 1)
    assert 0 < L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 3, 1, 0) < need <= ws.numel()
    assert L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 3, 1, 0) == L.ssd_conv3x3_train_workspace_bytes(lv(), 1, B, Cin, Cout)
    for what, rc, sized in (("k = 2", fwd(k=2), L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 2, 1, 0)),
                            ("stride 2 with k = 1", fwd(k=1, stride=2), L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 1, 2, 0)),
                            ("up with odd H", fwd(levels=lv(h=3), up_=ups), L.ssd_conv_train_workspace_bytes(lv(h=3), 1, B, Cin, Cout, 3, 1, 1)),
                            ("Cin = 6", fwd(k=1, cin=6), L.ssd_conv_train_workspace_bytes(lv(), 1, B, 6, Cout, 1, 1, 0)),
                            ("up with stride 2", fwd(stride=2, up_=ups), L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 3, 2, 1))):
        assert rc == -1 and sized == 0, what
    assert bwd(k=2) == -1 and bwd(k=1, stride=2) == -1 and bwd(k=1, cin=6) == -1
    assert bwd(k=1, o=dx) == -1 and b"1x1" in L.ssd_last_error()       # dx with k = 1
    assert fwd(up_=ups, wsb=need - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    short = L.ssd_conv_train_workspace_bytes(lv(), 1, B, Cin, Cout, 3, 2, 0)
    assert bwd(stride=2, o=dx, wsb=short - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    # the merge: null g, a bad flag, a misaligned pointer, out == g
    m = lambda base, g, gate, flag, o: L.ssd_fpn_merge_backward(base, g, gate, B, H // 2, W // 2, Cout, flag, o, s)
    assert m(None, None, None, 0, up.data_ptr()) == -1 and m(None, dy.data_ptr(), None, 2, up.data_ptr()) == -1
    assert m(None, dy.data_ptr() + 4, None, 0, up.data_ptr()) == -1 and m(None, up.data_ptr(), None, 1, up.data_ptr()) == -1
    cuda.cuda.synchronize()
    for t in (out, dx, dw):                                             # nothing ran
        assert bool((t == 7.0).all())
    assert fwd(up_=ups, wsb=need) == 0 and bwd(stride=1, o=dx) == 0      # and the same calls with good arguments run
    cuda.cuda.synchronize()
    assert bool((out == 0).all()) and bool((dw == 0).all())


# ----------------------------------------------------------------------------- 7. inference mode
def _engine_c(ssd, cuda, params, seed, keep=("p3", "p4", "p5", "p6", "p7")):
    W = ssd.synthetic_weights(params, seed=seed, logits_bias=-4.0)
    img = np.random.default_rng(seed + 1).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    eng = ssd.Engine(params, W, device=0)
    feats = ssd.BackboneFeatures(eng)(cuda.from_numpy(img).cuda())
    cs = [f.cpu().numpy() for f in feats]
    for name, c in zip(("c3", "c4", "c5"), cs):
        assert np.array_equal(c, eng.get_tensor(name))
    kept = {k: eng.get_tensor(k) for k in keep}
    eng.close()
    return W, img, cs, kept


@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_trainable_fpn_in_inference_mode_is_the_engine_bit_for_bit(ssd, cuda, backbone):
    params = dict(TINY_PARAMS, backbone=backbone)
    W, _, cs, kept = _engine_c(ssd, cuda, params, seed=11)
    assert cs[0].shape[3] == (116 if backbone == "shufflenet" else 256)
    m = ssd.TrainableFPN(params, W, device="cuda").eval()
    with cuda.no_grad():
        ps = m([_dev(cuda, c) for c in cs])
    assert [tuple(p.shape[1:3]) for p in ps] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    for l, p in zip(range(3, 8), ps):
        assert np.array_equal(p.cpu().numpy(), kept["p%d" % l]), l
        assert np.abs(kept["p%d" % l]).max() > 0


# ----------------------------------------------------------------------------- 8. training mode
def test_trainable_fpn_in_training_mode_against_the_float64_restatement(ssd, cuda):
    """Outputs, the gradient of sum(p_l * d_l) (d_l random, both signs) with respect to every variable, and the moving statistics,
    per tensor and norm-wise (head_train_ref.rel: max |got - ref64| / max |ref64|).  Reference: fpn() in float64 torch on the CPU
    with autograd and batch statistics.  Bound: the one test_predictor_in_training_mode_against_the_float64_restatement uses for
    the same quantities -- the figure of a float32 CPU torch run of the same graph is the yardstick, "the kernels get FACTOR = 4 x
    it".  The FPN's chains are shorter than the head's (at most three convolutions and one batch norm against five), so that is
    the margin.  Measured on an MI355X (profiles/r17_fpn_train.log): the kernels' figure equals the yardstick's to two digits on
    17 of the 33 tensors; the worst ratios are 3.9 x (d fpn/p3_batch_norm/gamma: 2.17e-6 against 5.56e-7) and 2.6 x (p3: 2.43e-6
    against 9.46e-7) -- the convolutions' pinned sequential fmaf chain over 2304 terms against torch's blocked float32 sums."""
    import torch
    FACTOR = 4.0
    W, _, cs, _ = _engine_c(ssd, cuda, TINY_PARAMS, seed=13, keep=())
    rng = np.random.default_rng(14)
    sizes = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    ds = [rng.normal(0, 1, (B, h, w, 256)).astype(f32) for h, w in sizes]
    runs = {}
    for dtype in (torch.float64, torch.float32):
        outs, T, S, p6 = ref.torch_fpn(W, cs, dtype)
        torch.autograd.backward(outs, [torch.tensor(d.astype(np.float64), dtype=dtype) for d in ds])
        rows = [("p%d" % (3 + l), outs[l].detach().numpy()) for l in range(5)]
        rows += [("d " + k, v.grad.numpy()) for k, v in T.items()] + [(k, v.numpy()) for k, v in S.items()]
        runs[dtype] = dict(rows)
    p6 = p6.detach().numpy()
    assert (p6 > 0).any() and (p6 <= 0).any()                           # a gate open and a gate closed: the ReLU between p6 and p7 matters
    m = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
    ps = m([_dev(cuda, c) for c in cs])
    cuda.autograd.backward(ps, [_dev(cuda, d) for d in ds])
    got = {"p%d" % (3 + l): ps[l].detach().cpu().numpy() for l in range(5)}
    got.update({"d " + k: v.grad.cpu().numpy() for k, v in m.named_variables().items()})
    got.update({k: v.cpu().numpy() for k, v in m.statistics().items()})
    assert set(got) == set(runs[torch.float64]) and len(got) == 5 + 18 + 10
    bad = []
    for name, r64 in runs[torch.float64].items():
        assert np.abs(r64).max() > 0, name                              # no vacuous comparison
        yard, d = ref.rel(runs[torch.float32][name], r64), ref.rel(got[name], r64)
        print("fpn train mode %-40s float32 torch %.3g  kernels %.3g" % (name, yard, d))
        if not d <= FACTOR * yard:
            bad.append((name, d, yard))
    assert not bad, bad
    for k, v in m.statistics().items():
        assert not np.array_equal(v.cpu().numpy(), W[k]), k


# ----------------------------------------------------------------------------- 9. the loop
def test_the_loop_closes_through_a_checkpoint(ssd, cuda, tmp_path):
    """Engine features -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward -> one TrainStep over both
    modules' variables -> save -> a fresh Detector on that checkpoint."""
    W, img, cs, _ = _engine_c(ssd, cuda, TINY_PARAMS, seed=17, keep=())
    anchors, boxes, labels, num = href.groundtruth(ssd, B, 19)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    fpn = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
    head = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").train()
    backbone = {k: v for k, v in W.items() if not k.startswith(("fpn/", "box_net/", "class_net/"))}
    assert backbone and len(backbone) + len(ssd.fpn_variable_shapes(TINY_PARAMS)) + len(ssd.head_variable_shapes(TINY_PARAMS)) == len(W)
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
    ts = ssd.TrainStep({**fpn.named_variables(), **head.named_variables()}, cfg, {**fpn.statistics(), **head.statistics()},
                       layout="tf", params=TINY_PARAMS, frozen=backbone)
    eb, cp = head(fpn([_dev(cuda, c) for c in cs]))
    out = ssd.differentiable_loss(cp, eb, _dev(cuda, anchors), gt, LP)
    (out["localization_loss"] + out["classification_loss"]).backward()
    for name, p in fpn.named_variables().items():
        assert p.grad is not None and bool(cuda.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    ts.step()
    ts.save(str(tmp_path))
    for name, p in fpn.named_variables().items():
        if name.endswith("/kernel"):
            assert not np.array_equal(p.detach().cpu().numpy(), W[name]), name
    saved = ssd.read_checkpoint(ssd.resolve_checkpoint(str(tmp_path)), list(backbone))
    for k, v in backbone.items():
        assert same_bits(saved[k], v), k
    with cuda.no_grad():
        want = fpn.eval()([_dev(cuda, c) for c in cs])[0].cpu().numpy()
    det = ssd.Detector(str(tmp_path), config=dict(TINY_PARAMS))
    det.engine.forward(cuda.from_numpy(img).cuda())
    assert np.array_equal(det.engine.get_tensor("c5"), cs[2])
    assert np.array_equal(det.engine.get_tensor("p3"), want)
    det.close()
