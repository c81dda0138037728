"""The TRAIN first convolution on the GPU (include/ssd_hip.h, "the TRAIN first convolution"): the raw forward against ssd_first_conv
and the CPU oracle bit for bit, the weight gradient exactly on integer dy and within the bound of a double sum rounded once on random
dy, its determinism, the last row and column, the refusals, TrainableMobileNet(train_first=True) in inference mode against the engine
bit for bit and in training mode against a float64 restatement with forced gates, the closed loop through a checkpoint with no frozen
variable, and the untouched default module."""
import numpy as np
import pytest

from helpers import backbone_train_ref as bref
from helpers import first_conv_train_ref as ref
from helpers import head_train_ref as href
from helpers.backbone_train_gpu import fc_backward_dev
from helpers.head_train_gpu import dev as _dev, same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
SIZES = [(2, 2), (4, 6), (6, 8), (10, 14), (32, 32)]                  # W % 4 == 0 and W % 4 == 2; (2,2): one output, ky = 2 and kx = 2 outside
WIDTHS = [8, 24, 32]
BATCHES = [1, 3]
LP = {"gamma": 2.0, "alpha": 0.25}
FIRST = "MobilenetV1/Conv2d_0"


def _images(rng, B, H, W):
    """Random bytes with 0, 127, 128 and 255 planted on the last row and the last column."""
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    plant = np.array([0, 127, 128, 255], np.uint8)
    img[:, H - 1, :, :] = plant[rng.integers(0, 4, (B, W, 3))]
    img[:, :, W - 1, :] = plant[rng.integers(0, 4, (B, H, 3))]
    return img


def _dw_raw(ssd, cuda, images, dy, fill_ws=None):
    """helpers.backbone_train_gpu.fc_backward_dev (a workspace of exactly the planner's size, dw pre-filled with NaN) on numpy arrays."""
    return fc_backward_dev(ssd, cuda, cuda.from_numpy(images).cuda(), _dev(cuda, dy), fill_ws).cpu().numpy()


# ----------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Cout", WIDTHS)
def test_forward_is_ssd_first_conv_and_the_oracle_bit_for_bit(ssd, cuda, oracle_ops, Cout, B):
    rng = np.random.default_rng(Cout + B)
    for H, W in SIZES:
        img = _images(rng, B, H, W)
        k = rng.normal(0, 0.5, (3, 3, 3, Cout)).astype(f32)
        timg = cuda.from_numpy(img).cuda()
        y = ssd.first_conv_train(timg, _dev(cuda, k))
        assert tuple(y.shape) == (B, H // 2, W // 2, Cout)
        eng = ssd.ssd.first_conv(timg, k, bn=None, act=None)
        want = oracle_ops.conv2d(oracle_ops.preprocess(img), k, stride=2)
        assert cuda.equal(y, eng), (H, W)
        assert same_bits(y.cpu().numpy(), want) and np.abs(want).max() > 0, (H, W)


# ----------------------------------------------------------------------------- 2. the weight gradient
def _exact_case(ssd, cuda, B, H, W, Cout, seed):
    """Integer dy in [-8, 8]: every term is a multiple of 2^-24 (test_first_conv_train_host.py) of magnitude at most 8, so a sum of R
    of them stays below R * 2^27 units of 2^-24 -- far below 2^53 for these shapes (asserted) --, every double addition is exact
    in any order, and dw must be float32(the float64 sum) on every element."""
    rng = np.random.default_rng(seed)
    img = _images(rng, B, H, W)
    dy = rng.integers(-8, 9, (B, H // 2, W // 2, Cout)).astype(f32)
    terms = ref.fc_terms(img, dy)
    units = terms * 2.0 ** 24
    assert np.array_equal(units, np.round(units)) and np.abs(units).sum(0).max() < 2.0 ** 53
    want = terms.sum(0).reshape(3, 3, 3, Cout)
    dw = _dw_raw(ssd, cuda, img, dy)
    assert dw.shape == want.shape and same_bits(dw, want.astype(f32)), (B, H, W, Cout)
    return want


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Cout", WIDTHS)
def test_weight_gradient_is_exact_on_integer_dy(ssd, cuda, Cout, B):
    for H, W in SIZES:
        want = _exact_case(ssd, cuda, B, H, W, Cout, Cout * 100 + B * 10 + H)
        assert np.abs(want).max() > 0
        if (H, W) == (2, 2):
            assert not want[2].any() and not want[:, 2].any()


def test_weight_gradient_is_exact_over_two_slabs(ssd, cuda):
    """B = 2 on 32 x 32 with 32 channels: R = 512 output rows, rpp = 32 row lanes, two slabs of 256 rows."""
    assert ref.slab_plan(512, 32) == (32, 256, 2)
    assert ssd.train_calls.first_conv_workspace_bytes((2, 32, 32), 32) == 2 * 27 * 32 * 8
    assert np.abs(_exact_case(ssd, cuda, 2, 32, 32, 32, 5)).max() > 0


def test_weight_gradient_is_exact_with_a_ragged_last_slab(ssd, cuda):
    """B = 3 on 10 x 14: R = 105 rows.  24 channels: rpp = 42, one slab of 336 rows with 105 in it (lanes of 3 and 2 rows); 32
    channels: one slab of 256; 8 channels: rpp = 128, one slab of 1024 -- 23 row lanes without a row."""
    for Cout, plan in ((24, (42, 336, 1)), (32, (32, 256, 1)), (8, (128, 1024, 1))):
        assert ref.slab_plan(105, Cout) == plan
        assert np.abs(_exact_case(ssd, cuda, 3, 10, 14, Cout, 6 + Cout)).max() > 0
    # and three slabs, the last with 2 rows: 2 frames of 2 x 514, 32 channels -> R = 514 = 256 + 256 + 2
    assert ref.slab_plan(514, 32) == (32, 256, 3)
    assert np.abs(_exact_case(ssd, cuda, 2, 2, 514, 32, 9)).max() > 0


@pytest.mark.parametrize("Cout", [24, 32])
def test_weight_gradient_obeys_the_bound_of_a_double_sum_rounded_once(ssd, cuda, Cout):
    """Random float dy: |dw - fl32(exact sum)| <= n 2^-53 sum|term| + one float32 ulp per element (head_train_ref.double_sum_bound):
    the products are exact in double, so only the order of the double additions and one rounding remain.  Two calls give the same
    bits; a workspace pre-filled with NaN changes nothing."""
    rng = np.random.default_rng(Cout)
    for H, W in [(10, 14), (32, 32)]:
        img = _images(rng, 3, H, W)
        dy = rng.normal(0, 1, (3, H // 2, W // 2, Cout)).astype(f32)
        terms = ref.fc_terms(img, dy)
        dw = _dw_raw(ssd, cuda, img, dy)
        assert np.isfinite(dw).all() and np.abs(dw).max() > 0             # the NaN pre-fill is fully overwritten
        worst = 0.0
        for t in range(27):
            want, tol = href.double_sum_bound(terms[:, t, :])
            err = np.abs(dw.reshape(27, Cout)[t].astype(f64) - want.astype(f64))
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (H, W, t, float((err / tol).max()))
        print("first conv dw Cout=%d %dx%d: worst |dw - exact| / bound = %.3g" % (Cout, H, W, worst))
        assert same_bits(dw, _dw_raw(ssd, cuda, img, dy))
        assert same_bits(dw, _dw_raw(ssd, cuda, img, dy, fill_ws=0xFF))    # 0xFF bytes: every double of the workspace a NaN


def test_the_last_row_and_column_matter(ssd, cuda):
    """A byte at [b, H-1, W-1, ci] is seen by tap (1,1) of the last output only; a byte at row H-2 by ky = 0 of the last output row
    and ky = 2 of the row above.  dy has no zero, so every tap that can see the byte moves; the kernel equals the reference before
    and after."""
    rng = np.random.default_rng(11)
    B, H, W, Cout = 2, 10, 14, 8
    img = _images(rng, B, H, W)
    dy = rng.choice(np.array([-3, -2, -1, 1, 2, 3], f32), (B, H // 2, W // 2, Cout))
    exact = lambda im: ref.fc_terms(im, dy).sum(0).reshape(3, 3, 3, Cout).astype(f32)
    base = _dw_raw(ssd, cuda, img, dy)
    assert same_bits(base, exact(img))
    ci = 1
    corner = img.copy()
    corner[1, H - 1, W - 1, ci] ^= 0x55
    got = _dw_raw(ssd, cuda, corner, dy)
    assert same_bits(got, exact(corner))
    moved = np.argwhere(got != base)
    assert len(moved) == Cout and all(tuple(m[:3]) == (1, 1, ci) for m in moved)
    above = img.copy()
    above[0, H - 2, W - 2, ci] ^= 0x55                                   # column W-2: kx = 0 of the last output column, kx = 2 of the one before
    got = _dw_raw(ssd, cuda, above, dy)
    assert same_bits(got, exact(above))
    moved = {tuple(m[:3]) for m in np.argwhere(got != base)}
    assert moved == {(0, 0, ci), (0, 2, ci), (2, 0, ci), (2, 2, ci)}


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals_come_before_any_launch(ssd, cuda):
    L = ssd.lib()
    B, H, W, C = 2, 6, 8, 8
    img = cuda.zeros((B, H, W, 3), dtype=cuda.uint8, device="cuda")
    w = cuda.zeros((3, 3, 3, C), device="cuda")
    dy = cuda.zeros((B, H // 2, W // 2, C), device="cuda")
    out, dw = cuda.full((B, H // 2, W // 2, C), 7.0, device="cuda"), cuda.full((3, 3, 3, C), 7.0, device="cuda")
    ws = cuda.empty(1 << 20, dtype=cuda.uint8, device="cuda")
    s = ssd.train_calls.stream(img.device)
    need = L.ssd_first_conv_train_workspace_bytes(B, H, W, C)
    assert 0 < need <= ws.numel()

    def fwd(b=B, h=H, ww=W, c=C, ip=img.data_ptr(), wp=w.data_ptr(), op=out.data_ptr()):
        return L.ssd_first_conv_train_forward(ip, b, h, ww, wp, c, op, s)

    def bwd(b=B, h=H, ww=W, c=C, ip=img.data_ptr(), dyp=dy.data_ptr(), dwp=dw.data_ptr(), wsp=ws.data_ptr(), wsb=ws.numel()):
        return L.ssd_first_conv_train_backward(ip, dyp, b, h, ww, c, dwp, wsp, wsb, s)
    sized = L.ssd_first_conv_train_workspace_bytes
    for what, kw, word in (("odd H", dict(h=5), b"even"), ("odd W", dict(ww=7), b"even"),
                           ("Cout = 6", dict(c=6), b"Cout"), ("Cout = 68", dict(c=68), b"Cout"), ("Cout = 0", dict(c=0), b"Cout"),
                           ("B = 0", dict(b=0), b"positive"), ("H = 0", dict(h=0), b"positive"), ("W = -2", dict(ww=-2), b"positive"),
                           ("2^31 bytes", dict(b=65536, h=128, ww=128), b"2^31")):
        assert fwd(**kw) == -1 and word in L.ssd_last_error(), what
        assert bwd(**kw) == -1 and word in L.ssd_last_error(), what
        assert sized(kw.get("b", B), kw.get("h", H), kw.get("ww", W), kw.get("c", C)) == 0, what
    for kw in (dict(ip=None), dict(wp=None), dict(op=None)):
        assert fwd(**kw) == -1 and b"null" in L.ssd_last_error(), kw
    for kw in (dict(ip=None), dict(dyp=None), dict(dwp=None), dict(wsp=None)):
        assert bwd(**kw) == -1 and b"null" in L.ssd_last_error(), kw
    for kw in (dict(wp=w.data_ptr() + 4), dict(op=out.data_ptr() + 8)):
        assert fwd(**kw) == -1 and b"16-byte" in L.ssd_last_error(), kw
    for kw in (dict(dyp=dy.data_ptr() + 4), dict(dwp=dw.data_ptr() + 4), dict(wsp=ws.data_ptr() + 8)):
        assert bwd(**kw) == -1 and b"16-byte" in L.ssd_last_error(), kw
    assert fwd(ip=img.data_ptr() + 2) == -1 and b"4-byte" in L.ssd_last_error()
    assert bwd(ip=img.data_ptr() + 1) == -1 and b"4-byte" in L.ssd_last_error()
    assert bwd(wsb=need - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    cuda.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dw == 7.0).all())         # nothing ran
    assert fwd() == 0 and bwd(wsb=need) == 0                            # and the same calls with good arguments run
    cuda.cuda.synchronize()
    assert bool((out == 0).all()) and bool((dw == 0).all())
    # the op: a kernel on the GPU whose images are not, and the other way round
    with pytest.raises(TypeError, match="GPU"):
        ssd.first_conv_train(img.cpu(), w)
    with pytest.raises(TypeError, match="GPU"):
        ssd.first_conv_train(img, w.cpu())


# ----------------------------------------------------------------------------- 4. the module
B = 2


def _engine(ssd, cuda, seed):
    W = ssd.synthetic_weights(TINY_PARAMS, seed=seed, logits_bias=-4.0)
    img = np.random.default_rng(seed + 1).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    eng = ssd.Engine(TINY_PARAMS, W, device=0)
    eng.forward(cuda.from_numpy(img).cuda())
    kept = {k: eng.get_tensor(k) for k in ("c3", "c4", "c5")}
    eng.close()
    return W, img, kept


def test_train_first_in_inference_mode_is_the_engine_and_the_default_module_bit_for_bit(ssd, cuda):
    W, img, kept = _engine(ssd, cuda, 61)
    timg = cuda.from_numpy(img).cuda()
    m = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", keep_features=True, train_first=True).eval()
    d = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda").eval()
    assert len(m.named_variables()) == 81 and len(m.statistics()) == 54 and m.frozen_variables() == {}
    assert {FIRST + "/weights", FIRST + "/BatchNorm/gamma", FIRST + "/BatchNorm/beta"} <= set(m.named_variables())
    assert {FIRST + "/BatchNorm/moving_mean", FIRST + "/BatchNorm/moving_variance"} <= set(m.statistics())
    with cuda.no_grad():
        cs, ds = m(timg), d(timg)
        x0 = d.first_conv(timg)
    for name, c, c_default in zip(("c3", "c4", "c5"), cs, ds):
        assert np.array_equal(c.cpu().numpy(), kept[name]) and np.abs(kept[name]).max() > 0, name
        assert cuda.equal(c, c_default), name
    assert len(m.features) == 27 and cuda.equal(m.features["Conv2d_0"], x0) and float(x0.max()) > 0
    for k, v in m.statistics().items():                                 # inference mode moves nothing
        assert same_bits(v.cpu().numpy(), W[k]), k


def test_train_first_in_training_mode_against_the_float64_restatement(ssd, cuda):
    """The whole backbone from the uint8 frames on batch statistics: c3, c4, c5, the gradient of sum(c_l * d_l) with respect to all 81
    variables, and the 54 moving statistics, per tensor and norm-wise (head_train_ref.rel) against the float64 CPU torch restatement
    of test_gpu_backbone_train.py extended by Conv2d_0, the ReLU6 gates forced to the run's own (Conv2d_0's from
    features["Conv2d_0"]).  Bound: at most FACTOR = 4 x the figure of a float32 CPU torch run with the same gates, the project's
    factor for the same quantities.  Measured on an MI355X (profiles/r20_first_conv_train.log): the worst
    ratios are 1.86 x (d Conv2d_4_pointwise/BatchNorm/gamma: 1.35e-5 against 7.27e-6; Conv2d_10_depthwise's moving variance) and
    d Conv2d_0/weights is at 1.24 x (1.61e-5 against 1.30e-5)."""
    import torch
    FACTOR = 4.0
    W = ssd.synthetic_weights(TINY_PARAMS, seed=71, logits_bias=-4.0)
    img = np.random.default_rng(72).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    m = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", keep_features=True, train_first=True).train()
    rng = np.random.default_rng(73)
    ds = [rng.normal(0, 1, (B, h, h, c)).astype(f32) for h, c in ((16, 256), (8, 512), (4, 1024))]
    cs = m(cuda.from_numpy(img).cuda())
    cuda.autograd.backward(cs, [_dev(cuda, d) for d in ds])
    feats = {k: v.cpu().numpy() for k, v in m.features.items()}
    gates = bref.gates_of(feats)
    assert len(gates) == 27 and gates["Conv2d_0"][0].any() and (~gates["Conv2d_0"][0]).any()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        outs, T, S = ref.torch_mobilenet_from_images(W, img, dtype, gates)
        torch.autograd.backward(outs, [torch.tensor(d.astype(f64), dtype=dtype) for d in ds])
        rows = [("c%d" % (3 + l), outs[l].detach().numpy()) for l in range(3)]
        rows += [("d " + k, v.grad.numpy()) for k, v in T.items()] + [(k, v.numpy()) for k, v in S.items()]
        runs[dtype] = dict(rows)
    got = {"c%d" % (3 + l): cs[l].detach().cpu().numpy() for l in range(3)}
    got.update({"d " + k: v.grad.cpu().numpy() for k, v in m.named_variables().items()})
    got.update({k: v.cpu().numpy() for k, v in m.statistics().items()})
    assert set(got) == set(runs[torch.float64]) and len(got) == 3 + 81 + 54
    bad, worst = [], (0.0, None)
    for name, r64 in runs[torch.float64].items():
        assert np.abs(r64).max() > 0, name                              # no vacuous comparison
        yard, d = bref.rel(runs[torch.float32][name], r64), bref.rel(got[name], r64)
        print("mobilenet train_first %-56s float32 torch %.3g  kernels %.3g  ratio %.2f" % (name, yard, d, d / yard))
        worst = max(worst, (d / yard, name))
        if not d <= FACTOR * yard:
            bad.append((name, d, yard))
    key = "d " + FIRST + "/weights"
    r64 = runs[torch.float64][key]
    print("mobilenet train_first worst ratio %.2f (%s)" % worst)
    print("mobilenet train_first ratio of %s: %.2f" % (key, bref.rel(got[key], r64) / bref.rel(runs[torch.float32][key], r64)))
    assert not bad, bad
    for k, v in m.statistics().items():                                 # every moving statistic moved, Conv2d_0's included
        assert not np.array_equal(v.cpu().numpy(), W[k]), k


def test_the_loop_closes_with_no_frozen_variable(ssd, cuda, tmp_path):
    """images -> TrainableMobileNet(train_first=True) -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward -> one
    TrainStep(frozen={}) over every variable of the model -> save -> a fresh Detector on that checkpoint."""
    W = ssd.synthetic_weights(TINY_PARAMS, seed=81, logits_bias=-4.0)
    img = cuda.from_numpy(np.random.default_rng(82).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)).cuda()
    anchors, boxes, labels, num = href.groundtruth(ssd, B, 83)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    backbone = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", train_first=True).train()
    fpn = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda").train()
    head = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").train()
    frozen = backbone.frozen_variables()
    assert frozen == {}
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
    variables = {**backbone.named_variables(), **fpn.named_variables(), **head.named_variables()}
    statistics = {**backbone.statistics(), **fpn.statistics(), **head.statistics()}
    assert len(variables) + len(statistics) == len(W)
    ts = ssd.TrainStep(variables, cfg, statistics, layout="tf", params=TINY_PARAMS, frozen=frozen)
    eb, cp = head(fpn(backbone(img)))
    out = ssd.differentiable_loss(cp, eb, _dev(cuda, anchors), gt, LP)
    (out["localization_loss"] + out["classification_loss"]).backward()
    for name, p in variables.items():
        assert p.grad is not None and bool(cuda.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    ts.step()
    ts.save(str(tmp_path))
    first = [FIRST + "/weights", FIRST + "/BatchNorm/gamma", FIRST + "/BatchNorm/beta", FIRST + "/BatchNorm/moving_mean",
             FIRST + "/BatchNorm/moving_variance"]
    saved = ssd.read_checkpoint(ssd.resolve_checkpoint(str(tmp_path)), first)
    now = {**backbone.named_variables(), **backbone.statistics()}
    for k in first:                                                     # the checkpoint holds the updated Conv2d_0, not the initial one
        assert same_bits(saved[k], now[k].detach().cpu().numpy()) and not np.array_equal(saved[k], W[k]), k
    with cuda.no_grad():
        cs = backbone.eval()(img)
        want_c5 = cs[2].cpu().numpy()
        want_p3 = fpn.eval()(cs)[0].cpu().numpy()
    det = ssd.Detector(str(tmp_path), config=dict(TINY_PARAMS))
    det.engine.forward(img)
    assert np.array_equal(det.engine.get_tensor("c5"), want_c5) and np.abs(want_c5).max() > 0
    assert np.array_equal(det.engine.get_tensor("p3"), want_p3)
    det.close()


def test_the_default_module_is_untouched(ssd, cuda):
    """train_first=False: 78 variables, 5 frozen arrays, and one forward and backward gives the same bits as a second run -- with
    Conv2d_1's depthwise asked for no data gradient, as before."""
    W = ssd.synthetic_weights(TINY_PARAMS, seed=91, logits_bias=-4.0)
    img = cuda.from_numpy(np.random.default_rng(92).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)).cuda()
    rng = np.random.default_rng(93)
    ds = [_dev(cuda, rng.normal(0, 1, (B, h, h, c)).astype(f32)) for h, c in ((16, 256), (8, 512), (4, 1024))]
    runs = []
    for _ in range(2):
        m = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", train_first=False).train()
        assert len(m.named_variables()) == 78 and len(m.statistics()) == 52 and len(m.frozen_variables()) == 5
        assert not any(k.startswith(FIRST + "/") for k in m.named_variables())
        x0 = m.first_conv(img)
        assert not x0.requires_grad
        cs = m(img)
        cuda.autograd.backward(cs, ds)
        runs.append(([c.detach().cpu().numpy() for c in cs], {k: v.grad.cpu().numpy() for k, v in m.named_variables().items()},
                     {k: v.cpu().numpy() for k, v in m.statistics().items()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert same_bits(a, b)
    for i in (1, 2):
        for k, v in runs[0][i].items():
            assert same_bits(v, runs[1][i][k]) and np.abs(v).max() > 0, k
    for k, v in m.frozen_variables().items():
        assert same_bits(v, W[k]), k
