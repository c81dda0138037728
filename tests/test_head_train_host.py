"""The TRAIN head, host side (no GPU): the float64 helper (tests/helpers/head_train_ref.py) against CPU torch autograd of an
independent float64 restatement (F.conv2d, F.batch_norm(training=True), relu); the argument checks of the six entry points;
TrainableBoxPredictor's variable names and shapes."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import head_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _weights(rng, nc, levels, C=8):
    W = {}
    for net, last, cout in (("box_net", "encoded_boxes", 24), ("class_net", "logits", 6 * nc)):
        for i in range(4):
            W["%s/conv3x3_%d/kernel" % (net, i)] = rng.normal(0, 0.2, (3, 3, C, C))
            for l in range(levels):
                s = "%s/batch_norm_%d_for_level_%d" % (net, i, 3 + l)
                W[s + "/gamma"] = rng.uniform(0.5, 1.5, C)
                W[s + "/beta"] = rng.normal(0, 0.3, C)
                W[s + "/moving_mean"] = rng.normal(0, 0.1, C)
                W[s + "/moving_variance"] = rng.uniform(0.5, 1.5, C)
        W["%s/%s/kernel" % (net, last)] = rng.normal(0, 0.1, (3, 3, C, cout))
        W["%s/%s/bias" % (net, last)] = rng.normal(0, 0.1, cout)
    return W


def _torch_predictor(W, feats, nc, dtype=torch.float64):
    """An independent float64 restatement in NCHW torch ops; returns outputs and {name: leaf}."""
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=not k.endswith(("moving_mean", "moving_variance"))) for k, v in W.items()}
    P = [torch.tensor(f.astype(np.float64), dtype=dtype, requires_grad=True) for f in feats]
    outs = []
    for net, last, width in (("box_net", "encoded_boxes", 4), ("class_net", "logits", nc)):
        ys = []
        for l, p in enumerate(P):
            x = p.permute(0, 3, 1, 2)
            for i in range(4):
                x = F.conv2d(x, T["%s/conv3x3_%d/kernel" % (net, i)].permute(3, 2, 0, 1), padding=1)
                s = "%s/batch_norm_%d_for_level_%d" % (net, i, 3 + l)
                if x.shape[0] * x.shape[2] * x.shape[3] > 1:
                    x = F.relu(F.batch_norm(x, None, None, T[s + "/gamma"], T[s + "/beta"], training=True, eps=ref.EPS))
                else:           # F.batch_norm refuses one value per channel in training mode: the same formula in plain ops
                    m = x.mean((0, 2, 3), keepdim=True)
                    v = ((x - m) ** 2).mean((0, 2, 3), keepdim=True)
                    x = F.relu((x - m) / torch.sqrt(v + ref.EPS) * T[s + "/gamma"][None, :, None, None] + T[s + "/beta"][None, :, None, None])
            x = F.conv2d(x, T["%s/%s/kernel" % (net, last)].permute(3, 2, 0, 1), T["%s/%s/bias" % (net, last)], padding=1)
            ys.append(x.permute(0, 2, 3, 1).reshape(p.shape[0], -1, width))
        outs.append(torch.cat(ys, 1))
    return outs, T, P


# an odd-sized level (5 x 7), a pyramid, and a level with R = 1 (one image, 1 x 1)
@pytest.mark.parametrize("B,sizes,nc", [(2, [(5, 7)], 3), (2, [(6, 4), (3, 2), (2, 1)], 2), (1, [(5, 7), (1, 1)], 1)])
def test_helper_equals_torch_autograd(B, sizes, nc):
    rng = np.random.default_rng(len(sizes) * 10 + nc)
    W = _weights(rng, nc, len(sizes))
    feats = [rng.normal(0, 1, (B, h, w, 8)) for h, w in sizes]
    boxes, classes = ref.predictor(W, feats, nc)
    d_boxes, d_classes = rng.normal(0, 1, boxes.shape), rng.normal(0, 1, classes.shape)
    grads, dfeats = ref.predictor(W, feats, nc, d_boxes=d_boxes, d_classes=d_classes)
    (tb, tc), T, P = _torch_predictor(W, feats, nc)
    assert _rel(boxes, tb.detach().numpy()) <= 1e-10 and _rel(classes, tc.detach().numpy()) <= 1e-10
    ((tb * torch.tensor(d_boxes)).sum() + (tc * torch.tensor(d_classes)).sum()).backward()
    trainable = [k for k in W if not k.endswith(("moving_mean", "moving_variance"))]
    assert set(grads) == set(trainable)
    lone = [l for l, (h, w) in enumerate(sizes) if B * h * w == 1]          # R = 1: xhat == 0, so dgamma and dx vanish identically (and with dx every gradient below the level's last batch norm)
    for k in trainable:
        want = T[k].grad.numpy()
        if np.abs(want).max() < 1e-12:
            assert "for_level" in k and int(k.split("for_level_")[1][0]) - 3 in lone, k
            assert np.abs(grads[k]).max() < 1e-12, k
            continue
        assert _rel(grads[k], want) <= 1e-10, k
    for l, p in enumerate(P):
        if l in lone:
            assert np.abs(dfeats[l]).max() < 1e-12 and np.abs(p.grad.numpy()).max() < 1e-12
            continue
        assert np.abs(p.grad.numpy()).max() > 0
        assert _rel(dfeats[l], p.grad.numpy()) <= 1e-10, l


def test_data_gradient_is_the_convolution_with_the_rotated_transposed_kernel():
    rng = np.random.default_rng(3)
    x, w, dy = rng.normal(0, 1, (2, 5, 7, 8)), rng.normal(0, 1, (3, 3, 8, 6)), rng.normal(0, 1, (2, 5, 7, 6))
    dxs, _, _ = ref.conv_grads([x], w, [dy])
    assert _rel(ref.conv(dy, ref.rotated_transposed(w)), dxs[0]) <= 1e-13


def _conv_call(L, which, a):
    lv = (a["cls"] * len(a["lv"]))(*a["lv"]) if a["lv"] is not None else None
    if which == "forward":
        return L.ssd_conv3x3_train_forward(lv, a["n"], a["B"], a["Cin"], a["Cout"], a["w"], a["bias"], a["ws"], a["wsb"], None)
    return L.ssd_conv3x3_train_backward(lv, a["n"], a["B"], a["Cin"], a["Cout"], a["w"], a["dw"], a["dbias"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_conv_entry_points_refuse_bad_arguments_without_a_gpu(ssd, which):
    """One defect per call; every call is refused before any HIP call (include/ssd_hip.h)."""
    L = ssd.lib()
    Lv = ssd._lib.SsdConvLevel
    P = ctypes.c_void_p

    def level(**kw):
        d = dict(H=5, W=7, x=0x10000, dy=0x20000, out=0x30000)
        d.update(kw)
        return Lv(d["H"], d["W"], d["x"], d["dy"], d["out"])
    two = [level(), level(H=3, W=4, x=0x40000, dy=0x50000, out=0x60000)]
    need = L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 2, 2, 64, 40)
    assert need > 0
    good = dict(cls=Lv, lv=two, n=2, B=2, Cin=64, Cout=40, w=P(0x70000), bias=None, dw=P(0x80000), dbias=None, ws=P(0x100000), wsb=need)
    defects = [dict(lv=None), dict(n=0), dict(n=9, lv=two * 5), dict(B=0), dict(Cin=0), dict(Cout=0), dict(Cin=60), dict(w=None), dict(ws=None),
               dict(wsb=need - 1), dict(w=P(0x70004)), dict(ws=P(0x100008)), dict(bias=P(0x90002)) if which == "forward" else dict(dbias=P(0x90002)),
               dict(lv=[level(H=0), two[1]]), dict(lv=[level(W=-1), two[1]]), dict(lv=[level(x=None), two[1]]), dict(lv=[level(x=0x10004), two[1]]),
               dict(lv=[level(out=0x30008), two[1]]), dict(B=1 << 20, lv=[level(H=1 << 10, W=1 << 10), two[1]])]
    if which == "forward":
        defects += [dict(lv=[level(out=None), two[1]])]
    else:
        defects += [dict(dw=None), dict(dw=P(0x80004)), dict(lv=[level(dy=None), two[1]]), dict(lv=[level(dy=0x20004), two[1]]),
                    dict(lv=[level(out=None), two[1]])]             # dx for one level only
    for d in defects:
        rc = _conv_call(L, which, dict(good, **d))
        assert rc == -1, d
        assert ("ssd_conv3x3_train_" + which).encode() in L.ssd_last_error(), d
    assert L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 2, 2, 60, 40) == 0
    assert L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 0, 2, 64, 40) == 0
    # widths up to the documented 4096 are planned (6 * num_classes passes 1024 from 171 classes on), wider ones refused
    for cout in (1028, 1030, 4096):
        wide = L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 2, 2, 64, cout)
        assert wide > need, cout
        assert _conv_call(L, which, dict(good, Cout=cout, wsb=wide - 1)) == -1 and b"workspace too small" in L.ssd_last_error()
    assert L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 2, 2, 64, 4100) == 0
    assert L.ssd_conv3x3_train_workspace_bytes((Lv * 2)(*two), 2, 2, 4104, 40) == 0
    for d in (dict(Cout=4100), dict(Cin=4104)):
        assert _conv_call(L, which, dict(good, **d)) == -1 and b"4096" in L.ssd_last_error(), d


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_batch_norm_entry_points_refuse_bad_arguments_without_a_gpu(ssd, which):
    L = ssd.lib()
    Lv = ssd._lib.SsdBnLevel
    P = ctypes.c_void_p
    names = ("x", "dy", "out", "gamma", "beta", "moving_mean", "moving_variance", "mean", "var", "invstd", "dgamma", "dbeta")

    def level(rows=35, **kw):
        d = {n: 0x10000 * (i + 1) for i, n in enumerate(names)}
        d.update(kw)
        return Lv(rows, *[d[n] for n in names])
    two = [level(), level(rows=1)]
    C = 256
    need = L.ssd_bn_relu_train_workspace_bytes((Lv * 2)(*two), 2, C)
    assert need > 0
    good = dict(lv=two, n=2, C=C, training=1, eps=1e-3, omm=0.007, ws=P(0x1000000), wsb=need)
    required = ("x", "out", "gamma", "beta", "mean", "invstd") + (() if which == "forward" else ("dy", "dgamma", "dbeta"))
    defects = [dict(lv=None), dict(n=0), dict(n=9, lv=two * 5), dict(C=0), dict(C=1025), dict(ws=None), dict(ws=P(0x1000004)), dict(wsb=need - 1),
               dict(lv=[level(rows=0), two[1]]), dict(lv=[level(rows=-3), two[1]])]
    defects += [dict(lv=[level(**{n: None}), two[1]]) for n in required]
    defects += [dict(lv=[two[0], level(rows=1, **{n: 0x10000 * (i + 1) + 4})]) for i, n in enumerate(names) if n in required]
    if which == "forward":
        defects += [dict(eps=0.0), dict(omm=-0.5), dict(omm=1.5), dict(training=2), dict(lv=[level(moving_mean=None), two[1]]),
                    dict(training=0, lv=[level(moving_mean=None, moving_variance=None), two[1]])]
    for d in defects:
        a = dict(good, **d)
        lv = (Lv * len(a["lv"]))(*a["lv"]) if a["lv"] is not None else None
        if which == "forward":
            rc = L.ssd_bn_relu_train_forward(lv, a["n"], a["C"], a["training"], a["eps"], a["omm"], a["ws"], a["wsb"], None)
        else:
            rc = L.ssd_bn_relu_train_backward(lv, a["n"], a["C"], a["ws"], a["wsb"], None)
        assert rc == -1, d
        assert ("ssd_bn_relu_train_" + which).encode() in L.ssd_last_error(), d
    assert L.ssd_bn_relu_train_workspace_bytes((Lv * 2)(*two), 2, 0) == 0


@pytest.mark.parametrize("config", ["config_mobilenet.json", "config_shufflenet.json"])
def test_predictor_variables_are_the_heads_subset_of_variable_shapes(ssd, config):
    params = ssd.load_config(os.path.join(ROOT, "tests", "golden", config))
    shapes = ssd.variable_shapes(params)
    head = {k: tuple(v) for k, v in shapes.items() if k.startswith(("box_net/", "class_net/"))}
    assert len(head) == 2 * (4 + 2 + 4 * 5 * 4)
    rng = np.random.default_rng(0)
    W = {k: rng.normal(0, 1, v).astype(np.float32) for k, v in head.items()}
    m = ssd.TrainableBoxPredictor(params, W)
    got = {k: tuple(v.shape) for k, v in m.named_variables().items()}
    got.update({k: tuple(v.shape) for k, v in m.statistics().items()})
    assert got == head
    assert list(m.named_variables()) + list(m.statistics()) != [] and set(m.named_variables()).isdisjoint(m.statistics())
    assert all(k.endswith(("moving_mean", "moving_variance")) for k in m.statistics()) and len(m.statistics()) == 80
    assert np.array_equal(m.variable("box_net/conv3x3_2/kernel").detach().numpy(), W["box_net/conv3x3_2/kernel"])
    # a new class list: class_net/logits takes the reference's initialiser, everything else is kept
    p2 = dict(params, num_classes=params["num_classes"] + 3)
    m2 = ssd.TrainableBoxPredictor(p2, W, seed=5)
    k2 = m2.variable("class_net/logits/kernel").detach().numpy()
    assert k2.shape == (3, 3, 256, 6 * p2["num_classes"]) and 0.008 < k2.std() < 0.012
    assert np.all(m2.variable("class_net/logits/bias").detach().numpy() == np.float32(-np.log(99.0)))
    assert np.array_equal(m2.variable("class_net/conv3x3_0/kernel").detach().numpy(), W["class_net/conv3x3_0/kernel"])


def test_torch_loss_restatement_equals_the_float64_loss_gradient_helper():
    """helpers.head_train_ref.torch_loss (the loss of the whole-graph runs of tests/test_gpu_head_train.py) in float64 has the
    gradient of tests/helpers/loss_grad_ref.py."""
    from helpers import loss_grad_ref
    rng = np.random.default_rng(0)
    cells = []
    for size in (0.25, 0.5):
        for cy in np.arange(size / 2, 1.0, size / 2):
            for cx in np.arange(size / 2, 1.0, size / 2):
                cells.append([cy - size / 2, cx - size / 2, cy + size / 2, cx + size / 2])
    anchors = np.array(cells, np.float32)
    N = len(anchors)
    boxes = np.zeros((2, 2, 4), np.float32)
    boxes[0] = [[0.0, 0.0, 0.3, 0.3], [0.5, 0.5, 1.0, 1.0]]
    boxes[1, 0] = [0.2, 0.2, 0.7, 0.75]
    labels, num = rng.integers(0, 3, (2, 2)).astype(np.int32), np.array([2, 1], np.int32)
    lg, cd = rng.normal(-1, 3, (2, N, 3)).astype(np.float32), rng.normal(0, 1.5, (2, N, 4)).astype(np.float32)
    x, c = torch.tensor(lg.astype(np.float64), requires_grad=True), torch.tensor(cd.astype(np.float64), requires_grad=True)
    total, least = ref.torch_loss(x, c, anchors, boxes, labels, num)
    total.backward()
    dl, dc = loss_grad_ref.batch_grads(lg, cd, anchors, boxes, labels, num)
    assert least >= 1 and np.abs(dl).max() > 0 and np.abs(dc).max() > 0
    assert _rel(x.grad.numpy(), dl) <= 1e-12 and _rel(c.grad.numpy(), dc) <= 1e-12


# ----------------------------------------------------------------------------- the references of tests/test_gpu_head_train_edges.py
def test_double_sum_bound_holds_for_any_order_of_double_summation_and_not_for_float32():
    """helpers.head_train_ref.double_sum_bound: a sequential float64 sum in a shuffled order and a long-double sum (math.fsum
    where long double is no wider), each rounded once to float32, stay inside it -- on ordinary columns, on a column that
    cancels to 2^-30 against terms that add up to 3e3 in magnitude, on an all-zero column.  A sequential float32 accumulation of the same terms does not:
    the bound separates the header's "sums in double, rounded ONCE" from a float32 sum."""
    import math
    rng = np.random.default_rng(1)
    n = 5000
    t = rng.normal(0, 1, (n, 6)).astype(np.float32).astype(np.float64) * rng.normal(0, 1, (n, 6)).astype(np.float32).astype(np.float64)
    t[n // 2:, 4] = -t[:n // 2, 4][::-1]                                 # cancels exactly ...
    t[0, 4] += 2.0 ** -30                                                 # ... but for this
    t[:, 5] = 0.0
    want, tol = ref.double_sum_bound(t)
    assert want[5] == 0 and abs(float(want[4]) - 2.0 ** -30) <= tol[4] and tol[4] < 1e-12 * np.abs(t[:, 4]).sum()
    for seed in range(5):
        order = np.random.default_rng(seed).permutation(n)
        seq = np.cumsum(t[order], axis=0)[-1].astype(np.float32)          # one addition at a time, in this order
        assert np.all(np.abs(seq.astype(np.float64) - want.astype(np.float64)) <= tol), seed
    if np.finfo(np.longdouble).nmant > 52:
        wide = t.astype(np.longdouble).sum(0).astype(np.float32)
    else:
        wide = np.array([math.fsum(t[:, c]) for c in range(6)], np.float32)
    assert np.all(np.abs(wide.astype(np.float64) - want.astype(np.float64)) <= tol)
    low = np.cumsum(t.astype(np.float32), axis=0, dtype=np.float32)[-1]
    assert np.any(np.abs(low.astype(np.float64) - want.astype(np.float64))[:4] > tol[:4])
    bad, _ = ref.double_sum_bound(np.where(np.arange(6) == 2, np.inf, t))
    assert np.isnan(bad[2]) and np.array_equal(np.delete(bad, 2), np.delete(want, 2))


def test_gate_and_restatement_agree_and_a_fused_multiply_add_does_not():
    """bn_gate_f32 forms the gate from the SAME float32 expression as bn_relu_f32's y; on these inputs a fused t * sf + beta (one
    rounding) differs from the header's two roundings in some elements: the bit-for-bit comparison of y can see a contraction."""
    rng = np.random.default_rng(2)
    x, dy = rng.normal(0.3, 1.5, (442, 256)).astype(np.float32), rng.normal(0, 1, (442, 256)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, 256).astype(np.float32), rng.normal(0, 0.3, 256).astype(np.float32)
    mean, var = x.astype(np.float64).mean(0).astype(np.float32), x.astype(np.float64).var(0).astype(np.float32)
    y, dx, dg, db = ref.bn_relu_f32(x, gamma, beta, mean, var, dy)
    g, xh = ref.bn_gate_f32(x, gamma, beta, mean, var, dy)
    assert np.array_equal(g != 0, (y > 0) & (dy != 0))
    y2, dx2, _, _ = ref.bn_relu_f32(x, gamma, beta, mean, var, dy, dgamma=dg, dbeta=db)
    assert np.array_equal(y, y2) and np.array_equal(dx, dx2)
    sf = gamma * ref.invstd_f32(var)
    fused = np.maximum(((x - mean).astype(np.float64) * sf.astype(np.float64) + beta.astype(np.float64)).astype(np.float32), 0)
    assert 0 < np.count_nonzero(fused != y) < y.size // 2
    # var = 0: the header's two float32 operations give the float32 just below fp32(1 / sqrt(eps)) rounded once
    two = ref.invstd_f32(np.zeros(1, np.float32))[0]
    once = np.float32(1.0 / np.sqrt(float(np.float32(ref.EPS))))
    assert two != once and abs(int(two.view(np.int32)) - int(once.view(np.int32))) == 1


def test_offset_channel_two_pass_variance_is_inside_the_bound_and_one_pass_is_not():
    """mean 1e3, std 1e-2 (the offset channels of the GPU test): the float64 variance around the float32 mean, rounded once, is
    within offset_variance_bound of the true float64 variance; E[x^2] - mean32^2 (sums in double) and an all-float32 one-pass
    variance are outside it by orders of magnitude."""
    rng = np.random.default_rng(5)
    x = (1e3 + 1e-2 * rng.normal(0, 1, (442, 3))).astype(np.float32)
    x64 = x.astype(np.float64)
    true = x64.var(0)
    m32 = x64.mean(0).astype(np.float32)
    bound = ref.offset_variance_bound(1e3, true.max())
    assert 1e-5 < bound < 1e-3
    two = ((x64 - m32.astype(np.float64)) ** 2).mean(0).astype(np.float32)
    assert np.all(np.abs(two.astype(np.float64) - true) / true <= bound)
    assert np.any(m32.astype(np.float64) != x64.mean(0))
    one = (x64 ** 2).mean(0) - m32.astype(np.float64) ** 2
    one32 = (x * x).mean(0, dtype=np.float32) - m32 * m32
    assert np.all(np.abs(one - true) / true > 100 * bound) and np.all(np.abs(one32.astype(np.float64) - true) / true > 100 * bound)


def test_slab_and_slice_formulas_give_what_the_cases_intend():
    assert ref.slab_plan([143360, 35840, 8960, 2240, 560], 256) == (4, 188, 1017)
    assert ref.slab_plan([442], 256) == (4, 32, 14) and ref.slab_plan([30], 6) == (128, 1024, 1)
    assert ref.rows_per_slice([17920, 4480, 1026], 256, 40) == 288 and ref.rows_per_slice([17920, 4480, 1026], 64, 40) == 256
    B, sizes, Cin, Cout = ref.CONV_CASES["slice-edge"]
    rows = [B * h * w for h, w in sizes]
    assert rows == [512, 513] and ref.rows_per_slice(rows, Cin, Cout) == 256


@pytest.mark.parametrize("case", sorted(ref.CONV_CASES))
def test_sweep_cases_keep_their_integer_premise(case):
    """What keeps the GPU sweep's exactness check sound: every absolute partial sum of the integer data is below 2^24 and the
    expected dw is not zero; the random data's bound is finite and positive."""
    B, sizes, Cin, Cout = ref.CONV_CASES[case]
    _, _, xs, w, bias, dys = ref.conv_case_data(case, integers=True)
    assert Cin % 8 == 0 and all(x.shape == (B, h, ww, Cin) for x, (h, ww) in zip(xs, sizes)) and 1 <= len(sizes) <= 8
    assert max(np.abs(x).max() for x in xs) <= 3 and max(np.abs(d).max() for d in dys) <= 3 and np.abs(w).max() <= 2
    dw64, db64, top_w, top_b = ref.integer_premise(xs, w, dys)
    assert top_w < 2 ** 24 and top_b < 2 ** 24 and np.abs(dw64).max() > 0 and np.abs(db64).max() > 0
    _, _, xs, w, bias, dys = ref.conv_case_data(case, integers=False)
    dw64, bound, absum = ref.wgrad_bound(xs, w, dys)
    assert np.all(bound > 0) and np.all(np.isfinite(bound)) and np.all(np.abs(dw64) <= absum)


def test_large_predictor_input_has_a_yardstick_for_every_tensor(ssd):
    """The 320 x 448 input of the GPU test: at least one match per image, every reference tensor non-zero and every float32
    yardstick above zero, so that FACTOR x yardstick is a bound and no comparison is vacuous."""
    from conftest import TINY_PARAMS
    W, feats, anchors, boxes, labels, num = ref.large_predictor_input(ssd, TINY_PARAMS)
    assert [f.shape for f in feats] == [(3, h, w, 256) for h, w in ref.LARGE_SIZES]
    assert anchors.shape[0] == sum(6 * h * w for h, w in ref.LARGE_SIZES)
    least, rows = ref.predictor_references(W, feats, anchors, boxes, labels, num)
    assert least >= 1 and len(rows) == 2 + 2 * (4 + 2 + 4 * 5 * 2) + 5
    for name, t32, r64 in rows:
        assert np.abs(r64).max() > 0, name
        yard = ref.rel(t32, r64)
        print("yardstick 320x448 %-48s %.3g" % (name, yard))
        assert 0 < yard < 1e-2, name
