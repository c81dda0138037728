"""GPU-side helpers shared by tests/test_gpu_head_train.py, tests/test_gpu_head_train_edges.py and tests/test_gpu_fpn_train.py: the
training entry points (include/ssd_hip.h, "the TRAIN head" and "the TRAIN FPN") through ssd.train_calls, autograd runs of
conv_same, and the body of the predictor's training-mode comparison."""
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


def bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys=None, training=1, fill=float("nan"), workspace=True, act=None):
    """ssd_bn_relu_train_forward (and, with dys, _backward) through ssd.train_calls -- act "relu" or "relu6": ssd_bn_act_train_*
    with that act; returns per level dicts of numpy arrays.
    Every output is pre-filled with `fill`; the statistics sit in rows padded to a multiple of 4 channels, so that every pointer
    is 16-byte aligned for any C.  workspace=False passes NULL (inference mode does not use it)."""
    calls = ssd.train_calls
    n, C = len(xs), xs[0].shape[-1]
    Cp = (C + 3) // 4 * 4
    t = lambda a: dev(cuda, a)
    X, G, Bt, MM, MV = [t(v) for v in xs], [t(v) for v in gammas], [t(v) for v in betas], [t(v) for v in mms], [t(v) for v in mvs]
    Y = [cuda.full_like(v, fill) for v in X]
    st = cuda.full((n, 5, Cp), fill, device="cuda")
    mean, var, invstd, dgamma, dbeta = [[st[i, j] for i in range(n)] for j in range(5)]
    ws = cuda.empty(max(calls.bn_workspace_bytes(X, C), 256) if workspace else 0, dtype=cuda.uint8, device="cuda")
    how = dict(workspace=ws, entry="bn_relu") if act is None else dict(workspace=ws, entry="bn_act", act=act)
    calls.bn_forward(X, Y, G, Bt, training, float(f32(ref.EPS)), float(f32(1.0 - ref.MOMENTUM)), MM, MV, mean, var, invstd, **how)
    out = [dict(y=Y[i].cpu().numpy(), mean=st[i, 0, :C].cpu().numpy(), var=st[i, 1, :C].cpu().numpy(), invstd=st[i, 2, :C].cpu().numpy(),
                mm=MM[i].cpu().numpy(), mv=MV[i].cpu().numpy()) for i in range(n)]
    if dys is not None:
        DX = [cuda.full_like(v, fill) for v in X]
        calls.bn_backward(X, [t(v) for v in dys], DX, G, Bt, mean, invstd, dgamma, dbeta, **how)
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


def exact_workspace(cuda, need, fill_ws=None):
    """A workspace of exactly `need` bytes, the planner's, pre-filled with the byte `fill_ws` when given."""
    assert need > 0
    return cuda.empty(need, dtype=cuda.uint8, device="cuda") if fill_ws is None else cuda.full((need,), fill_ws, dtype=cuda.uint8, device="cuda")


def _conv_workspace(ssd, cuda, xs, Wt, general, stride, fill_ws=None):
    """general: the call is ssd_conv_train_* with k from the kernel, `stride` and no up, else ssd_conv3x3_train_*.  -> (its
    exact_workspace, its entry)."""
    k, _, Cin, Cout = Wt.shape
    entry = "conv" if general else "conv3x3"
    return exact_workspace(cuda, ssd.train_calls.conv_workspace_bytes(xs, xs[0].shape[0], Cin, Cout, k, stride, entry=entry), fill_ws), entry


def conv_forward_raw(ssd, cuda, xs, w, bias, general=False, stride=1):
    """The forward through ssd.train_calls (general: see _conv_workspace); outputs pre-filled with NaN.  -> ([y], workspace bytes)."""
    X, Wt = [dev(cuda, x) for x in xs], dev(cuda, w)
    Y = [cuda.full((x.shape[0], -(-x.shape[1] // stride), -(-x.shape[2] // stride), w.shape[3]), float("nan"), device="cuda") for x in xs]
    ws, entry = _conv_workspace(ssd, cuda, X, Wt, general, stride)
    ssd.train_calls.conv_forward(X, Wt, Y, stride, dev(cuda, bias) if bias is not None else None, workspace=ws, entry=entry)
    return [y.cpu().numpy() for y in Y], ws.numel()


def conv_backward_raw(ssd, cuda, xs, w, dys, with_dx, with_dbias, sentinel=-7.5, general=False, stride=1, fill_ws=None):
    """The backward through ssd.train_calls (general, fill_ws: see _conv_workspace): dxs = None unless with_dx, dbias = None unless
    with_dbias.  -> ([dx] or None, dw, the dbias buffer -- pre-filled with `sentinel`, passed to the call only with_dbias)."""
    X, DY, Wt = [dev(cuda, x) for x in xs], [dev(cuda, d) for d in dys], dev(cuda, w)
    DX = [cuda.full_like(x, float("nan")) for x in X] if with_dx else None
    dw = cuda.full_like(Wt, float("nan"))
    db = cuda.full(((w.shape[3] + 3) // 4 * 4,), sentinel, device="cuda")
    ws, entry = _conv_workspace(ssd, cuda, X, Wt, general, stride, fill_ws)
    ssd.train_calls.conv_backward(X, Wt, DY, dw, stride, DX, db if with_dbias else None, workspace=ws, entry=entry)
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
