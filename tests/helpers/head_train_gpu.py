"""GPU-side helpers shared by tests/test_gpu_head_train.py, tests/test_gpu_head_train_edges.py and tests/test_gpu_fpn_train.py: the
training entry points straight through the C ABI (include/ssd_hip.h, "the TRAIN head" and "the TRAIN FPN"), autograd runs of
conv_same, and the body of the predictor's training-mode comparison."""
import ctypes

import numpy as np

from helpers import head_train_ref as ref

f32 = np.float32


def dev(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a, dtype=f32)).cuda()


def ulps(a, b):
    """Distance in units of the last place between float32 arrays of one sign pattern."""
    ia, ib = a.astype(f32).view(np.int32).astype(np.int64), b.astype(f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def same_bits(a, b):
    """Bit equality of two float32 arrays (0.0 and -0.0 differ; a NaN equals only the same NaN)."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


ACT = {"relu": 1, "relu6": 2}


def stream(cuda):
    return ctypes.c_void_p(cuda.cuda.current_stream().cuda_stream)


def bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys=None, training=1, fill=float("nan"), workspace=True, act=None):
    """ssd_bn_relu_train_forward (and, with dys, _backward) straight through the C ABI -- act "relu" or "relu6": ssd_bn_act_train_*
    with that act; returns per level dicts of numpy arrays.
    Every output is pre-filled with `fill`; the statistics sit in rows padded to a multiple of 4 channels, so that every pointer
    is 16-byte aligned for any C.  workspace=False passes NULL (inference mode does not use it)."""
    L = ssd.lib()
    n, C = len(xs), xs[0].shape[-1]
    Cp = (C + 3) // 4 * 4
    t = lambda a: dev(cuda, a)
    X, G, Bt, MM, MV = [t(v) for v in xs], [t(v) for v in gammas], [t(v) for v in betas], [t(v) for v in mms], [t(v) for v in mvs]
    Y = [cuda.full_like(v, fill) for v in X]
    st = cuda.full((n, 5, Cp), fill, device="cuda")
    DX = [cuda.full_like(v, fill) for v in X]
    DY = [t(v) for v in dys] if dys is not None else [None] * n
    lv = (ssd._lib.SsdBnLevel * n)()
    for i in range(n):
        lv[i].rows = X[i].numel() // C
        for name, v in (("x", X[i]), ("dy", DY[i]), ("out", Y[i]), ("gamma", G[i]), ("beta", Bt[i]), ("moving_mean", MM[i]),
                        ("moving_variance", MV[i]), ("mean", st[i, 0]), ("var", st[i, 1]), ("invstd", st[i, 2]), ("dgamma", st[i, 3]),
                        ("dbeta", st[i, 4])):
            setattr(lv[i], name, v.data_ptr() if v is not None else None)
    ws = cuda.empty(max(L.ssd_bn_relu_train_workspace_bytes(lv, n, C), 256), dtype=cuda.uint8, device="cuda")
    wsp, wsb = (ws.data_ptr(), ws.numel()) if workspace else (None, 0)
    family, acts = ("ssd_bn_relu_train_", ()) if act is None else ("ssd_bn_act_train_", (ACT[act],))
    s = stream(cuda)
    ssd._lib.check(getattr(L, family + "forward")(lv, n, C, *acts, training, float(f32(ref.EPS)), float(f32(1.0 - ref.MOMENTUM)), wsp, wsb, s))
    out = [dict(y=Y[i].cpu().numpy(), mean=st[i, 0, :C].cpu().numpy(), var=st[i, 1, :C].cpu().numpy(), invstd=st[i, 2, :C].cpu().numpy(),
                mm=MM[i].cpu().numpy(), mv=MV[i].cpu().numpy()) for i in range(n)]
    if dys is not None:
        for i in range(n):
            lv[i].out = DX[i].data_ptr()
        ssd._lib.check(getattr(L, family + "backward")(lv, n, C, *acts, wsp, wsb, s))
        for i in range(n):
            out[i].update(dx=DX[i].cpu().numpy(), dgamma=st[i, 3, :C].cpu().numpy(), dbeta=st[i, 4, :C].cpu().numpy())
    return out


def conv_backward(ssd, cuda, xs, w, dys, stride=1, bias=True, with_dx=True):
    """conv_same's gradients through autograd (bias: a zero bias is added): ([dx] or None, dw, dbias or None) as numpy."""
    tx = [dev(cuda, x).requires_grad_(with_dx) for x in xs]
    tw = dev(cuda, w).requires_grad_()
    tb = cuda.zeros(w.shape[3], device="cuda", requires_grad=True) if bias else None
    ys = ssd.conv_same(tx, tw, stride=stride, bias=tb)
    cuda.autograd.backward(ys, [dev(cuda, d) for d in dys])
    return [t.grad.cpu().numpy() for t in tx] if with_dx else None, tw.grad.cpu().numpy(), tb.grad.cpu().numpy() if bias else None


def _conv_raw(ssd, cuda, which, general, X, DY, OUT, Wt, stride, *ptrs, fill_ws=None):
    """One call of ssd_conv3x3_train_<which> -- general: of ssd_conv_train_<which> with k from the kernel, `stride` and, for the
    forward, up = NULL -- with a workspace of exactly the size its planner asks for, pre-filled with the byte `fill_ws` when given.
    -> that size."""
    L = ssd.lib()
    lv = (ssd._lib.SsdConvLevel * len(X))()
    for i, x in enumerate(X):
        lv[i].H, lv[i].W, lv[i].x = x.shape[1], x.shape[2], x.data_ptr()
        lv[i].dy, lv[i].out = DY[i].data_ptr() if DY else None, OUT[i].data_ptr() if OUT else None
    k, _, Cin, Cout = Wt.shape
    dims = (lv, len(X), X[0].shape[0], Cin, Cout)
    need = L.ssd_conv_train_workspace_bytes(*dims, k, stride, 0) if general else L.ssd_conv3x3_train_workspace_bytes(*dims)
    assert need > 0
    ws = cuda.empty(need, dtype=cuda.uint8, device="cuda") if fill_ws is None else cuda.full((need,), fill_ws, dtype=cuda.uint8, device="cuda")
    tail = (ws.data_ptr(), ws.numel(), stream(cuda))
    if general:
        up = (None,) if which == "forward" else ()
        ssd._lib.check(getattr(L, "ssd_conv_train_" + which)(*dims, k, stride, Wt.data_ptr(), *ptrs, *up, *tail))
    else:
        ssd._lib.check(getattr(L, "ssd_conv3x3_train_" + which)(*dims, Wt.data_ptr(), *ptrs, *tail))
    return need


def conv_forward_raw(ssd, cuda, xs, w, bias, general=False, stride=1):
    """The forward straight through the C ABI (general: see _conv_raw); outputs pre-filled with NaN.  -> ([y], workspace bytes)."""
    X, Wt = [dev(cuda, x) for x in xs], dev(cuda, w)
    Y = [cuda.full((x.shape[0], -(-x.shape[1] // stride), -(-x.shape[2] // stride), w.shape[3]), float("nan"), device="cuda") for x in xs]
    tb = dev(cuda, bias) if bias is not None else None
    need = _conv_raw(ssd, cuda, "forward", general, X, None, Y, Wt, stride, tb.data_ptr() if bias is not None else None)
    return [y.cpu().numpy() for y in Y], need


def conv_backward_raw(ssd, cuda, xs, w, dys, with_dx, with_dbias, sentinel=-7.5, general=False, stride=1, fill_ws=None):
    """The backward straight through the C ABI (general, fill_ws: see _conv_raw): out = NULL for every level unless with_dx, dbias_dev
    = NULL unless with_dbias.  -> ([dx] or None, dw, the dbias buffer -- pre-filled with `sentinel`, passed to the call only with_dbias)."""
    X, DY, Wt = [dev(cuda, x) for x in xs], [dev(cuda, d) for d in dys], dev(cuda, w)
    DX = [cuda.full_like(x, float("nan")) for x in X] if with_dx else None
    dw = cuda.full_like(Wt, float("nan"))
    db = cuda.full(((w.shape[3] + 3) // 4 * 4,), sentinel, device="cuda")
    _conv_raw(ssd, cuda, "backward", general, X, DY, DX, Wt, stride, dw.data_ptr(), db.data_ptr() if with_dbias else None, fill_ws=fill_ws)
    return [d.cpu().numpy() for d in DX] if with_dx else None, dw.cpu().numpy(), db.cpu().numpy()


def predictor_training_check(ssd, cuda, params, loss_params, W, feats, anchors, boxes, labels, num, factor, tag):
    """TrainableBoxPredictor in training mode + differentiable_loss + one backward against helpers.head_train_ref.
    predictor_references: per tensor max |got - ref64| / max |ref64| of the kernels may be at most `factor` x the same figure of
    the float32 CPU torch run.  Both figures are printed per tensor."""
    least, refs = ref.predictor_references(W, feats, anchors, boxes, labels, num, params["num_classes"])
    assert least >= 1                                               # at least one match per image
    m = ssd.TrainableBoxPredictor(params, W, device="cuda").train()
    fx = [dev(cuda, f).requires_grad_() for f in feats]
    eb, cp = m(fx)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    out = ssd.differentiable_loss(cp, eb, dev(cuda, anchors), gt, loss_params)
    (out["localization_loss"] + out["classification_loss"]).backward()
    got = {"encoded_boxes": eb.detach().cpu().numpy(), "class_predictions": cp.detach().cpu().numpy()}
    got.update({"d " + name: p.grad.cpu().numpy() for name, p in m.named_variables().items()})
    got.update({"d p%d" % (3 + l): fx[l].grad.cpu().numpy() for l in range(len(feats))})
    assert set(got) == {name for name, _, _ in refs}
    bad = []
    for name, t32, r64 in refs:
        assert np.abs(r64).max() > 0, name                            # no vacuous comparison
        yard, d = ref.rel(t32, r64), ref.rel(got[name], r64)
        print("train mode %s %-48s float32 torch %.3g  kernels %.3g" % (tag, name, yard, d))
        if not d <= factor * yard:
            bad.append((name, d, yard))
    assert not bad, bad
