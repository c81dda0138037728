"""The TRAIN head on the GPU (include/ssd_hip.h, "the TRAIN head"): the convolution's forward against ssd_conv2d and its data
gradient against the CPU oracle bit for bit, the weight gradient exactly on integers and within the order-free fp32 bound on
random data, the batch norm against the float64 / float32 restatements of tests/helpers/head_train_ref.py, the predictor in
inference mode against the engine bit for bit and in training mode against the float64 restatement, and the closed training loop
with its checkpoint."""
import numpy as np
import pytest

from helpers import head_train_ref as ref
from helpers.head_train_gpu import bn_raw as _bn_raw, conv_backward as _backward, dev as _dev, predictor_training_check, ulps as _ulps
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(256, 256), (256, 24), (256, 480), (64, 40)]
PYRAMID = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]          # odd sizes; B = 2: 442 + 126 + 40 + 12 + 2 rows
B = 2
LP = {"gamma": 2.0, "alpha": 0.25}


def _levels(rng, sizes, C, integers=False):
    if integers:
        return [rng.integers(-3, 4, (B, h, w, C)).astype(f32) for h, w in sizes]
    return [rng.normal(0, 1, (B, h, w, C)).astype(f32) for h, w in sizes]


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_forward_is_ssd_conv2d_bit_for_bit(ssd, cuda, Cin, Cout):
    rng = np.random.default_rng(Cin + Cout)
    xs = _levels(rng, PYRAMID, Cin)
    w = rng.normal(0, 0.05, (3, 3, Cin, Cout)).astype(f32)
    bias = rng.normal(0, 0.1, Cout).astype(f32)
    for b in (None, bias):
        ys = ssd.conv3x3_same([_dev(cuda, x) for x in xs], _dev(cuda, w), None if b is None else _dev(cuda, b))
        for x, y in zip(xs, ys):
            want = ssd.ssd.conv2d(_dev(cuda, x), w, bias=b)
            assert y.shape == want.shape and cuda.equal(y, want), (x.shape, b is None)
    one = ssd.conv3x3_same(_dev(cuda, xs[1]), _dev(cuda, w))            # a tensor in, a tensor out
    assert cuda.equal(one, ssd.ssd.conv2d(_dev(cuda, xs[1]), w))


def test_conv3x3_same_refuses_what_it_refused(ssd, cuda):
    """A kernel that is not 3x3 and a level of another width are ValueErrors; a single tensor in gives a single tensor out."""
    x = cuda.zeros((B, 4, 6, 8), device="cuda")
    with pytest.raises(ValueError):
        ssd.conv3x3_same(x, cuda.zeros((1, 1, 8, 16), device="cuda"))
    with pytest.raises(ValueError):
        ssd.conv3x3_same([x, cuda.zeros((B, 4, 6, 12), device="cuda")], cuda.zeros((3, 3, 8, 16), device="cuda"))
    y = ssd.conv3x3_same(x, cuda.zeros((3, 3, 8, 16), device="cuda"))
    assert isinstance(y, cuda.Tensor) and tuple(y.shape) == (B, 4, 6, 16)


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_data_gradient_is_the_oracles_convolution_bit_for_bit(ssd, cuda, oracle_ops, Cin, Cout):
    rng = np.random.default_rng(Cin * 3 + Cout)
    xs, dys = _levels(rng, PYRAMID, Cin), _levels(rng, PYRAMID, Cout)
    w = rng.normal(0, 0.05, (3, 3, Cin, Cout)).astype(f32)
    dxs, _, _ = _backward(ssd, cuda, xs, w, dys)
    wr = ref.rotated_transposed(w)
    for dy, dx in zip(dys, dxs):
        want = oracle_ops.conv2d(dy, wr)
        assert np.array_equal(dx, want), dy.shape


@pytest.mark.parametrize("Cin,Cout", SHAPES)
@pytest.mark.parametrize("nlev", [1, 2, 5])
def test_weight_gradient_is_exact_on_small_integers(ssd, cuda, Cin, Cout, nlev):
    """|v| <= 3 integers: every partial sum is an integer below 2^24, so dw and dbias are exact in ANY order.  442 rows of the
    first level are no multiple of the K-step (16) or of the slice (256 rows at these sizes: two slices, the second partial)."""
    rng = np.random.default_rng(nlev * 1000 + Cin + Cout)
    sizes = PYRAMID[:nlev]
    xs, dys = _levels(rng, sizes, Cin, True), _levels(rng, sizes, Cout, True)
    w = rng.integers(-2, 3, (3, 3, Cin, Cout)).astype(f32)
    _, dw64, db64 = ref.conv_grads(xs, w, dys)
    _, absum, _ = ref.conv_grads(xs, w, dys, absolute=True)
    assert absum.max() < 2 ** 24 and sum(np.abs(d).sum((0, 1, 2)).max() for d in dys) < 2 ** 24       # the premise, checked
    assert np.abs(dw64).max() > 0
    _, dw, db = _backward(ssd, cuda, xs, w, dys)
    assert np.array_equal(dw.astype(np.float64), dw64)
    assert np.array_equal(db.astype(np.float64), db64)


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_weight_gradient_obeys_the_order_free_fp32_bound(ssd, cuda, Cin, Cout):
    """|dw - dw64| <= gamma_n * sum |x * dy| per element, n its number of products, gamma_n = n u / (1 - n u), u = 2^-24: the bound
    of ANY order of fp32 accumulation (derived, not measured).  Measured max |dw - dw64| / sum |x * dy|: profiles/r14_head_train.log."""
    rng = np.random.default_rng(Cin * 7 + Cout)
    xs, dys = _levels(rng, PYRAMID, Cin), _levels(rng, PYRAMID, Cout)
    w = rng.normal(0, 0.05, (3, 3, Cin, Cout)).astype(f32)
    _, dw64, db64 = ref.conv_grads(xs, w, dys)
    _, absum, _ = ref.conv_grads(xs, w, dys, absolute=True)
    ones = lambda c: [np.ones((B, h, ww, c)) for h, ww in PYRAMID]
    _, n, _ = ref.conv_grads(ones(Cin), w, ones(Cout))
    u = 2.0 ** -24
    bound = n * u / (1 - n * u) * absum
    _, dw, db = _backward(ssd, cuda, xs, w, dys)
    err = np.abs(dw.astype(np.float64) - dw64)
    print("wgrad %d->%d: max |dw - dw64| / sum|x dy| = %.3g (gamma_n up to %.3g)" % (Cin, Cout, (err / absum).max(), (n * u / (1 - n * u)).max()))
    assert np.all(err <= bound)
    # dbias: a double sum rounded once
    assert np.all(np.abs(db.astype(np.float64) - db64) <= np.abs(db64) * 2.0 ** -23 + 1e-30)
    _, dw2, db2 = _backward(ssd, cuda, xs, w, dys)
    assert np.array_equal(dw, dw2) and np.array_equal(db, db2)


@pytest.mark.parametrize("Cin,Cout", [(256, 40), (64, 40)])
def test_weight_gradient_is_exact_with_many_slices_per_level(ssd, cuda, Cin, Cout):
    """The slice arithmetic of production shapes: 23 426 rows in three levels.  256 -> 40 takes its slice from the block target
    (18 tiles: 85 slices wanted, 288 rows each: 63 + 16 + 4 slices, every level's last one partial), 64 -> 40 the floor of 256
    rows (70 + 18 + 5 slices, the first level an exact multiple).  Integers |v| <= 3 again, the premise checked."""
    rng = np.random.default_rng(Cin)
    sizes = [(80, 112), (40, 56), (19, 27)]
    xs, dys = _levels(rng, sizes, Cin, True), _levels(rng, sizes, Cout, True)
    w = rng.integers(-2, 3, (3, 3, Cin, Cout)).astype(f32)
    assert ssd.train_calls.conv_workspace_bytes(sizes, B, Cin, Cout, entry="conv3x3") > 0
    _, dw64, db64 = ref.conv_grads(xs, w, dys)
    _, absum, _ = ref.conv_grads(xs, w, dys, absolute=True)
    assert absum.max() < 2 ** 24 and sum(np.abs(d).sum((0, 1, 2)).max() for d in dys) < 2 ** 24
    _, dw, db = _backward(ssd, cuda, xs, w, dys)
    assert np.array_equal(dw.astype(np.float64), dw64) and np.array_equal(db.astype(np.float64), db64)


@pytest.mark.parametrize("Cout", [1028, 1030, 2056])
def test_layers_wider_than_1024_channels(ssd, cuda, Cout):
    """Cout above 1024 (6 * num_classes from 171 classes on): dbias's column sums take one block per 1024 channels; 1030 is no
    multiple of 4 (element-wise loads).  Integers: the forward, dx, dw and dbias are all exact."""
    rng = np.random.default_rng(Cout)
    sizes = [(6, 7), (3, 3)]
    xs, dys = _levels(rng, sizes, 8, True), _levels(rng, sizes, Cout, True)
    w = rng.integers(-2, 3, (3, 3, 8, Cout)).astype(f32)
    bias = rng.integers(-4, 5, Cout).astype(f32)
    ys = ssd.conv3x3_same([_dev(cuda, x) for x in xs], _dev(cuda, w), _dev(cuda, bias))
    for x, y in zip(xs, ys):
        assert np.array_equal(y.cpu().numpy().astype(np.float64), ref.conv(x, w, bias=bias))
    dx64, dw64, db64 = ref.conv_grads(xs, w, dys)
    assert max(np.abs(d).max() for d in dx64) < 2 ** 24 and np.abs(dw64).max() < 2 ** 24
    dxs, dw, db = _backward(ssd, cuda, xs, w, dys)
    for got, want in zip(dxs, dx64):
        assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(dw.astype(np.float64), dw64) and np.array_equal(db.astype(np.float64), db64)
    assert np.abs(db64[1024:]).max() > 0


def test_batch_norm_relu_with_a_channel_count_that_is_no_multiple_of_4(ssd, cuda):
    """batch_norm_relu through autograd for C = 6 (the element-wise path; the saved statistics sit in padded rows): y, dx, dgamma
    and dbeta against the float64 restatement, 1e-5 of each tensor's largest value (a float32 evaluation of a few dozen rows)."""
    rng = np.random.default_rng(6)
    C = 6
    x, dy = rng.normal(0.2, 1.0, (2, 3, 5, C)).astype(f32), rng.normal(0, 1, (2, 3, 5, C)).astype(f32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(f32), rng.normal(0, 0.3, C).astype(f32)
    tx, tg, tb = _dev(cuda, x).requires_grad_(), _dev(cuda, gamma).requires_grad_(), _dev(cuda, beta).requires_grad_()
    mm, mv = cuda.zeros(C, device="cuda"), cuda.ones(C, device="cuda")
    y = ssd.batch_norm_relu(tx, tg, tb, mm, mv, training=True)
    y.backward(_dev(cuda, dy))
    y64 = ref.bn_relu_forward(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))[0]
    dx64, dg64, db64 = ref.bn_relu_backward(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), dy)
    for got, want in ((y, y64), (tx.grad, dx64), (tg.grad, dg64), (tb.grad, db64)):
        assert np.abs(want).max() > 0
        assert np.abs(got.detach().cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert mm.abs().max().item() > 0


def test_batch_norm_against_the_restatements(ssd, cuda):
    """Mean and biased variance: the float64 value rounded once, 1 ulp allowed (the double sum's order).  invstd and the moving
    statistics: the float32 restatement applied to the kernel's mean and variance, bit for bit.  y, dx, dgamma, dbeta: within
    FACTOR = 4 x the distance of the float32 numpy restatement (header order) from the float64 one on these inputs.  Measured
    (max abs, float32 restatement / kernel): R = 442: y 8.1e-7 / 8.1e-7, dx 4.2e-7 / 4.2e-7, dgamma 2.1e-5 / 5.2e-6, dbeta
    1.8e-5 / 1.8e-6; R = 35: y 6.7e-7 / 6.7e-7, dx 7.1e-7 / 7.1e-7, dgamma 1.7e-6 / 9.8e-7, dbeta 1.6e-6 / 4.0e-7; R = 1: all 0 / 0
    (profiles/r14_head_train.log)."""
    FACTOR = 4.0
    rng = np.random.default_rng(11)
    C = 256
    shapes = [(2, 13, 17, C), (1, 5, 7, C), (1, 1, 1, C)]                  # R = 442, 35, 1
    xs = [(rng.normal(0.3, 1.5, s)).astype(f32) for s in shapes]
    dys = [rng.normal(0, 1, s).astype(f32) for s in shapes]
    gammas = [rng.uniform(0.5, 1.5, C).astype(f32) for _ in shapes]
    betas = [rng.normal(0, 0.3, C).astype(f32) for _ in shapes]
    mms = [rng.normal(0, 0.1, C).astype(f32) for _ in shapes]
    mvs = [rng.uniform(0.5, 1.5, C).astype(f32) for _ in shapes]
    got = _bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)
    again = _bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)
    for i, s in enumerate(shapes):
        R = s[0] * s[1] * s[2]
        x64 = xs[i].astype(np.float64)
        g = got[i]
        y64, mean64, var64, _ = ref.bn_relu_forward(x64, gammas[i].astype(np.float64), betas[i].astype(np.float64))
        dx64, dg64, db64 = ref.bn_relu_backward(x64, gammas[i].astype(np.float64), betas[i].astype(np.float64), dys[i])
        assert _ulps(g["mean"], mean64.astype(f32)).max() <= 1
        # (the kernel's sum runs around ITS float32 mean: that adds (mean32 - mean)^2 ~ 1e-15 var, far below the rounding)
        assert _ulps(g["var"], var64.astype(f32)).max() <= 1
        assert np.array_equal(g["invstd"], ref.invstd_f32(g["var"]))
        mm, mv = ref.moving_update(mms[i], mvs[i], g["mean"], g["var"], R)
        assert np.array_equal(g["mm"], mm) and np.array_equal(g["mv"], mv)
        assert not np.array_equal(g["mm"], mms[i])
        # the float32 restatement on the float64 statistics rounded once: the yardstick
        y32, dx32, dg32, db32 = ref.bn_relu_f32(xs[i], gammas[i], betas[i], mean64.astype(f32), var64.astype(f32), dys[i])
        for name, k, r32, r64 in (("y", g["y"], y32, y64), ("dx", g["dx"], dx32, dx64), ("dgamma", g["dgamma"], dg32, dg64),
                                  ("dbeta", g["dbeta"], db32, db64)):
            yard = np.abs(r32.astype(np.float64) - r64).max()
            dev = np.abs(k.astype(np.float64) - r64).max()
            print("batch norm R=%d %s: float32 restatement %.3g, kernel %.3g (allowed %.3g)" % (R, name, yard, dev, FACTOR * yard))
            assert np.isfinite(k).all() and dev <= FACTOR * yard, (R, name, dev, yard)
        for key in g:
            assert np.array_equal(g[key], again[i][key]), key


def _engine_features(ssd, cuda, seed=1, batch=2):
    W = ssd.synthetic_weights(TINY_PARAMS, seed=seed, logits_bias=-4.0)
    img = np.random.default_rng(seed + 1).integers(0, 256, (batch, 128, 128, 3), dtype=np.uint8)
    eng = ssd.Engine(TINY_PARAMS, W, device=0)
    eng.forward(cuda.from_numpy(img).cuda())
    feats = [eng.get_tensor("p%d" % l) for l in range(3, 8)]
    out = eng.get_tensor("encoded_boxes"), eng.get_tensor("class_predictions")
    eng.close()
    return W, feats, out


def test_predictor_in_inference_mode_is_the_engine_bit_for_bit(ssd, cuda):
    W, feats, (boxes, classes) = _engine_features(ssd, cuda)
    m = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").eval()
    with cuda.no_grad():
        eb, cp = m([_dev(cuda, f) for f in feats])
    N = ssd.AnchorGenerator()(128, 128).shape[0]
    assert tuple(eb.shape) == (2, N, 4) and tuple(cp.shape) == (2, N, 80)
    assert np.array_equal(eb.cpu().numpy().reshape(boxes.shape), boxes)
    assert np.array_equal(cp.cpu().numpy().reshape(classes.shape), classes)


_groundtruth = ref.groundtruth


def test_predictor_in_training_mode_against_the_float64_restatement(ssd, cuda):
    """Outputs and the gradient of differentiable_loss with respect to every variable and to p3 .. p7, per tensor and norm-wise
    (max |got - ref64| / max |ref64|; a ReLU input at zero may fall on the other side in another precision).  Reference: the
    float64 numpy restatement of the predictor, with the loss's gradient taken by float64 torch autograd at its float64 outputs.
    Yardstick: the same figure for a float32 CPU torch run of the same graph -- predictor and loss (helpers.head_train_ref.torch_loss)
    in float32 torch ops, one backward; the kernels get FACTOR = 4 x it.  Both figures are printed per tensor and recorded in
    profiles/r14_head_train.log.  Measured on an MI355X: the kernels' figure is at or below the yardstick on most of the 99
    tensors; the worst ratio is 2.2 x (d class_net/batch_norm_3_for_level_7/beta, two rows: 5.26e-7 against 2.38e-7)."""
    FACTOR = 4.0
    W, feats, _ = _engine_features(ssd, cuda, seed=3)
    predictor_training_check(ssd, cuda, TINY_PARAMS, LP, W, feats, *_groundtruth(ssd, 2, 5), factor=FACTOR, tag="128x128")


def _run_loop(ssd, cuda, W, feats, anchors, gt, steps, tmp=None, resume_from=None):
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
    m = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").train()
    ts = ssd.TrainStep(m.named_variables(), cfg, m.statistics(), layout="tf", params=TINY_PARAMS)
    if resume_from is not None:
        ts.restore(resume_from)
    fx = [_dev(cuda, f) for f in feats]
    a = _dev(cuda, anchors)
    losses = []
    for _ in range(steps):
        for p in m.parameters():
            p.grad = None
        eb, cp = m(fx)
        out = ssd.differentiable_loss(cp, eb, a, gt, LP)
        total = out["localization_loss"] + out["classification_loss"]
        total.backward()
        ts.step()
        losses.append(float(total.item()))
    return m, ts, losses


def _state(m, ts):
    s = {k: v.detach().cpu().numpy().copy() for k, v in m.named_variables().items()}
    s.update({k: v.cpu().numpy().copy() for k, v in m.statistics().items()})
    for k in ts.names:
        mm, vv = ts.slots(k)
        s["m/" + k], s["v/" + k], s["ema/" + k] = mm.cpu().numpy().copy(), vv.cpu().numpy().copy(), ts.ema(k).cpu().numpy().copy()
    return s


def test_the_loop_closes(ssd, cuda, tmp_path):
    """20 steps on one fixed batch: the loss falls, the moving statistics move, two runs give the same bits; save -> restore into
    a fresh predictor + TrainStep gives back every variable, statistic and slot, and step 21 continues bit for bit."""
    W, feats, _ = _engine_features(ssd, cuda, seed=7)
    anchors, boxes, labels, num = _groundtruth(ssd, 2, 9)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    _, _, matches = ssd.get_training_targets(_dev(cuda, anchors), boxes, labels, num)
    assert ((matches >= 0).sum(1) > 0).all()                           # at least one match per image
    m1, ts1, l1 = _run_loop(ssd, cuda, W, feats, anchors, gt, 20)
    print("loss step 1 %.6g, step 20 %.6g" % (l1[0], l1[-1]))
    assert l1[-1] < l1[0]
    s1 = _state(m1, ts1)
    moved = [k for k in m1.statistics() if not np.array_equal(s1[k], W[k])]
    assert len(moved) == len(m1.statistics())
    m2, ts2, l2 = _run_loop(ssd, cuda, W, feats, anchors, gt, 20)
    s2 = _state(m2, ts2)
    assert l1 == l2 and all(np.array_equal(s1[k], s2[k]) for k in s1)
    ts1.save(str(tmp_path))
    m3 = ssd.TrainableBoxPredictor(TINY_PARAMS, ssd.synthetic_weights(TINY_PARAMS, seed=99), device="cuda").train()
    ts3 = ssd.TrainStep(m3.named_variables(), ts1.config, m3.statistics(), layout="tf", params=TINY_PARAMS)
    ts3.restore(str(tmp_path))
    s3 = _state(m3, ts3)
    assert ts3.global_step == 20 and all(np.array_equal(s1[k], s3[k]) for k in s1)

    def one_more(m, ts):
        for p in m.parameters():
            p.grad = None
        eb, cp = m([_dev(cuda, f) for f in feats])
        out = ssd.differentiable_loss(cp, eb, _dev(cuda, anchors), gt, LP)
        (out["localization_loss"] + out["classification_loss"]).backward()
        ts.step()
        return _state(m, ts)
    a21, b21 = one_more(m1, ts1), one_more(m3, ts3)
    assert all(np.array_equal(a21[k], b21[k]) for k in a21)
