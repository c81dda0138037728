"""How a TRAIN entry point of include/ssd_hip.h is called ("the TRAIN head", "the TRAIN FPN", "the TRAIN backbone", "the TRAIN first
convolution" from uint8 and from float frames, "the TRAIN ShuffleNet", "the TRAIN step's norms", "the TRAIN step's gradient exchange"): the only module that fills ssd_conv_level / ssd_bn_level, orders the arguments, sizes the workspace and passes the
stream.  One function per entry point family, no autograd, no model.  Arguments are torch tensors, None exactly where the header
allows NULL; every result is the CALLER's tensor.  Before the library is called every tensor is checked against the shape the
geometry implies (ValueError naming the argument: shape, dtype, contiguity, level counts) and then for lying on one GPU
(TypeError: there is no CPU path); alignment and size limits stay the C side's refusals (SsdError).
workspace=None: the grow-only buffer per (device, stream), sized by the call's own planner; workspace=<uint8 tensor>: exactly that
buffer (data_ptr(), numel()), which the family's *_workspace_bytes sizes."""
import ctypes

import numpy as np
import torch

from ._lib import SsdBnLevel, SsdConvLevel, check, lib

ACTS = {"relu": 1, "relu6": 2}                                                 # SSD_ACT_RELU, SSD_ACT_RELU6
SN_ACTS = dict(ACTS, none=0)                                                   # entry "sn_bn" alone: SSD_ACT_NONE too
_workspaces = {}


def stream(device):
    """The current torch stream of `device` as the entry points' `void *stream`."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(device, nbytes):
    """A grow-only scratch buffer per (device, stream): every call is ordered on the stream that owns it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _need(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError("%s must be a float32 tensor on a GPU (there is no CPU path)" % name)


# ----------------------------------------------------------------------------- the checks
def _dense(t, name, shape, dtype=torch.float32):
    """t is a contiguous `dtype` tensor of `shape` (None: any size along that axis) -> its shape."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape)
            and all(want in (None, have) for want, have in zip(shape, t.shape))):
        raise ValueError("%s must be a contiguous %s tensor of shape %s" % (name, str(dtype)[6:], list(shape)))
    return t.shape


def _vector(t, name, C):
    """t is None or a per-channel vector, 1-D float32 contiguous with AT LEAST C elements (a padded row, a sentinel behind it)
    -> its address."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() >= C and t.is_contiguous()):
        raise ValueError("%s must be a contiguous 1-D float32 tensor of at least %d elements" % (name, C))
    return t.data_ptr()


def _levels(xs):
    xs = list(xs)
    if not 1 <= len(xs) <= 8:                                                  # SSD_TRAIN_MAX_LEVELS
        raise ValueError("xs: 1 .. 8 levels")
    return xs


def _column(col, name, shapes):
    """col is None or holds one dense tensor per level of `shapes` -> the list."""
    if col is None:
        return None
    col = list(col)
    if len(col) != len(shapes):
        raise ValueError("%s: one tensor for every one of the %d levels (or None for all of them)" % (name, len(shapes)))
    for i, (t, shape) in enumerate(zip(col, shapes)):
        _dense(t, "%s[%d]" % (name, i), shape)
    return col


def conv_out_shape(shape, Cout, stride):
    """The output shape of a 'same' convolution of an input of `shape` [B,H,W,C] at `stride`: [B,ceil(H/stride),ceil(W/stride),Cout]."""
    if not (isinstance(stride, int) and stride >= 1):
        raise ValueError("stride must be a positive integer")
    return (shape[0], -(-shape[1] // stride), -(-shape[2] // stride), Cout)


def _one_gpu(workspace, **tensors):
    """LAST of the checks, so that the others can be exercised on CPU tensors: every tensor (lists flattened, None skipped) and the
    caller's workspace, a 1-D uint8 tensor, on ONE GPU -> that device."""
    if workspace is not None:
        _dense(workspace, "workspace", (None,), torch.uint8)
    dev = None
    for name, v in dict(tensors, workspace=workspace).items():
        for t in (v if isinstance(v, (list, tuple)) else (v,)):
            if t is not None:
                if not t.is_cuda:
                    raise TypeError("%s must be on a GPU (there is no CPU path)" % name)
                if dev not in (None, t.device):
                    raise ValueError("%s is on %s, another argument on %s: one device per call" % (name, t.device, dev))
                dev = t.device
    return dev


def _run(dev, workspace, need, call):
    """call(workspace_dev, workspace_bytes, stream) on `dev`; need() -> the planner's bytes, asked only for the cached workspace."""
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else _workspace(dev, need())
        check(call(ws.data_ptr(), ws.numel(), stream(dev)))


# ----------------------------------------------------------------------------- the convolution
_CONV = {"conv": "ssd_conv_train_", "conv3x3": "ssd_conv3x3_train_", "pointwise": "ssd_pointwise_train_",
         "sn_pointwise": "ssd_sn_pointwise_train_"}                            # the TRAIN ShuffleNet's: any even Cin, Cout; forward too


def _conv_extra(entry, k, stride, with_up=False):
    """The arguments that only the general family takes; the other two fix them."""
    if entry == "conv":
        return (k, stride)
    if entry not in _CONV or (k, stride) != ((3, 1) if entry == "conv3x3" else (1, 1)) or with_up:
        raise ValueError("entry must be 'conv', 'conv3x3' (k = 3, stride 1, no ups) or 'pointwise' / 'sn_pointwise' (k = 1, stride 1, no ups)")
    return ()


def _conv_need(entry, dims, k, stride, with_up):
    return getattr(lib(), _CONV[entry] + "workspace_bytes")(*dims, *((k, stride, 1 if with_up else 0) if entry == "conv" else ()))


def conv_workspace_bytes(levels, B, Cin, Cout, k=3, stride=1, with_up=False, entry="conv"):
    """ssd_conv_train_workspace_bytes (entry "conv3x3", "pointwise": that family's planner): levels are (H, W) pairs or [B,H,W,C]
    tensors of which only H and W are read."""
    _conv_extra(entry, k, stride, with_up)
    sizes = [l.shape[1:3] if isinstance(l, torch.Tensor) else l for l in levels]
    return _conv_need(entry, ((SsdConvLevel * len(sizes))(*[SsdConvLevel(h, w) for h, w in sizes]), len(sizes), B, Cin, Cout), k, stride, with_up)


def _conv_args(xs, kernel, stride, entry, with_up=False):
    """The checks both convolution calls share -> (xs, B, Cin, Cout, k, the family's extra arguments, every level's output shape)."""
    xs = _levels(xs)
    k, _, Cin, Cout = _dense(kernel, "kernel", (None,) * 4)
    if kernel.shape[1] != k:
        raise ValueError("kernel must be HWIO [k,k,Cin,Cout]")
    extra = _conv_extra(entry, k, stride, with_up)
    B = _dense(xs[0], "xs[0]", (None, None, None, Cin))[0]
    return xs, B, Cin, Cout, k, extra, [conv_out_shape(_dense(x, "xs[%d]" % i, (B, None, None, Cin)), Cout, stride) for i, x in enumerate(xs)]


def _conv_levels(xs, dys, outs):
    lv = (SsdConvLevel * len(xs))()
    for i, x in enumerate(xs):
        lv[i].H, lv[i].W = x.shape[1], x.shape[2]
        lv[i].x = x.data_ptr()
        lv[i].dy = dys[i].data_ptr() if dys is not None else None
        lv[i].out = outs[i].data_ptr() if outs is not None else None
    return lv


def conv_forward(xs, kernel, outs, stride=1, bias=None, ups=None, workspace=None, entry="conv"):
    """ssd_conv_train_forward (entry "conv3x3": ssd_conv3x3_train_forward; "sn_pointwise": ssd_sn_pointwise_train_forward, k = 1, no
    bias, no ups) of the levels xs [B,H,W,Cin] with ONE kernel HWIO
    [k,k,Cin,Cout] into outs [B,ceil(H/stride),ceil(W/stride),Cout]; bias [Cout] and ups (one [B,H/2,W/2,Cout] per level) nullable."""
    if entry == "pointwise":
        raise ValueError("entry: the pointwise family has no forward of its own ('conv' runs a 1x1 kernel)")
    xs, B, Cin, Cout, k, extra, shapes = _conv_args(xs, kernel, stride, entry, ups is not None)
    outs = _column(outs, "outs", shapes)
    ups = _column(ups, "ups", [(B, x.shape[1] // 2, x.shape[2] // 2, Cout) for x in xs])
    if entry == "sn_pointwise" and bias is not None:
        raise ValueError("bias: the sn_pointwise family has none")
    middle = (_vector(bias, "bias", Cout),) if entry != "sn_pointwise" else ()
    dev = _one_gpu(workspace, xs=xs, kernel=kernel, outs=outs, bias=bias, ups=ups)
    if entry == "conv":
        middle += ((ctypes.c_void_p * len(xs))(*[u.data_ptr() for u in ups]) if ups is not None else None,)
    dims, fn = (_conv_levels(xs, None, outs), len(xs), B, Cin, Cout), getattr(lib(), _CONV[entry] + "forward")
    _run(dev, workspace, lambda: _conv_need(entry, dims, k, stride, ups is not None), lambda *tail: fn(*dims, *extra, kernel.data_ptr(), *middle, *tail))


def conv_backward(xs, kernel, dys, dw, stride=1, dxs=None, dbias=None, workspace=None, entry="conv"):
    """ssd_conv_train_backward (entry "conv3x3": ssd_conv3x3_train_backward; "pointwise" / "sn_pointwise": ssd_pointwise_train_backward
    / ssd_sn_pointwise_train_backward, k = 1 with the data gradient and no dbias) from xs, the kernel and dys (the forward's output shapes): dw of the kernel's shape, dxs (for
    every level or None) of the levels' shapes, dbias [Cout] nullable."""
    xs, B, Cin, Cout, k, extra, shapes = _conv_args(xs, kernel, stride, entry)
    dys = _column(dys, "dys", shapes)
    _dense(dw, "dw", kernel.shape)
    dxs = _column(dxs, "dxs", [x.shape for x in xs])
    if entry in ("pointwise", "sn_pointwise") and dbias is not None:
        raise ValueError("dbias: the pointwise families have none")
    middle = (dw.data_ptr(),) + ((_vector(dbias, "dbias", Cout),) if entry not in ("pointwise", "sn_pointwise") else ())
    dev = _one_gpu(workspace, xs=xs, kernel=kernel, dys=dys, dw=dw, dxs=dxs, dbias=dbias)
    dims, fn = (_conv_levels(xs, dys, dxs), len(xs), B, Cin, Cout), getattr(lib(), _CONV[entry] + "backward")
    _run(dev, workspace, lambda: _conv_need(entry, dims, k, stride, False), lambda *tail: fn(*dims, *extra, kernel.data_ptr(), *middle, *tail))


def fpn_merge_backward(g, base=None, gate=None, same_size=False, out=None):
    """ssd_fpn_merge_backward: out = base + the 2x2 sums of g [B,2H,2W,C] (same_size: + g [B,H,W,C]), the g terms read as +0 where
    gate > 0 is false; base None starts at +0.  out may be base (in place).  No autograd."""
    _need(g, "g")
    g = g.contiguous()
    B, H, W, C = g.shape
    if not same_size:
        if (H | W) & 1:
            raise ValueError("g must have even height and width")
        H, W = H // 2, W // 2
    for t, name in ((base, "base"), (gate, "gate"), (out, "out")):
        if t is not None:
            _need(t, name)
            if tuple(t.shape) != (B, H, W, C) or not t.is_contiguous():
                raise ValueError("%s must be a contiguous [B,H,W,C] tensor of the output's shape" % name)
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        check(lib().ssd_fpn_merge_backward(base.data_ptr() if base is not None else None, g.data_ptr(),
                                           gate.data_ptr() if gate is not None else None, B, H, W, C, 1 if same_size else 0,
                                           out.data_ptr(), stream(g.device)))
    return out


# ----------------------------------------------------------------------------- the depthwise and the first convolution
_DW = {"depthwise": "ssd_depthwise_train_", "sn_depthwise": "ssd_sn_depthwise_train_"}    # the TRAIN ShuffleNet's: any even C


def _dw_entry(entry, which):
    if entry not in _DW:
        raise ValueError("entry must be 'depthwise' or 'sn_depthwise'")
    return getattr(lib(), _DW[entry] + which)


def depthwise_forward(x, kernel, out, stride=1, entry="depthwise"):
    """ssd_depthwise_train_forward (entry "sn_depthwise": ssd_sn_depthwise_train_forward): x [B,H,W,C], kernel [3,3,C,1] -> out
    [B,ceil(H/stride),ceil(W/stride),C]."""
    fn = _dw_entry(entry, "forward")
    B, H, W, C = _dense(x, "x", (None,) * 4)
    _dense(kernel, "kernel", (3, 3, C, 1))
    _dense(out, "out", conv_out_shape(x.shape, C, stride))
    dev = _one_gpu(None, x=x, kernel=kernel, out=out)
    with torch.cuda.device(dev):
        check(fn(x.data_ptr(), B, H, W, C, kernel.data_ptr(), stride, out.data_ptr(), stream(dev)))


def depthwise_workspace_bytes(x, stride, entry="depthwise"):
    """ssd_depthwise_train_workspace_bytes (entry "sn_depthwise": ssd_sn_depthwise_train_workspace_bytes): x is the input or its shape
    (B, H, W, C)."""
    return _dw_entry(entry, "workspace_bytes")(*getattr(x, "shape", x), stride)


def depthwise_backward(x, kernel, dy, dw, stride=1, dx=None, workspace=None, entry="depthwise"):
    """ssd_depthwise_train_backward (entry "sn_depthwise": ssd_sn_depthwise_train_backward) from x, the kernel and dy (the forward's
    output shape): dw of the kernel's shape, dx of x's shape or None."""
    need, fn = _dw_entry(entry, "workspace_bytes"), _dw_entry(entry, "backward")
    B, H, W, C = _dense(x, "x", (None,) * 4)
    _dense(kernel, "kernel", (3, 3, C, 1))
    _dense(dy, "dy", conv_out_shape(x.shape, C, stride))
    _dense(dw, "dw", (3, 3, C, 1))
    if dx is not None:
        _dense(dx, "dx", x.shape)
    dev = _one_gpu(workspace, x=x, kernel=kernel, dy=dy, dw=dw, dx=dx)
    dxp = dx.data_ptr() if dx is not None else None
    _run(dev, workspace, lambda: need(B, H, W, C, stride),
         lambda *tail: fn(x.data_ptr(), dy.data_ptr(), B, H, W, C, kernel.data_ptr(), stride, dxp, dw.data_ptr(), *tail))


def first_conv_forward(images, kernel, out):
    """ssd_first_conv_train_forward: images uint8 [B,H,W,3], kernel [3,3,3,Cout] -> out [B,H/2,W/2,Cout]."""
    B, H, W, _ = _dense(images, "images", (None, None, None, 3), torch.uint8)
    Cout = _dense(kernel, "kernel", (3, 3, 3, None))[3]
    _dense(out, "out", (B, H // 2, W // 2, Cout))
    dev = _one_gpu(None, images=images, kernel=kernel, out=out)
    with torch.cuda.device(dev):
        check(lib().ssd_first_conv_train_forward(images.data_ptr(), B, H, W, kernel.data_ptr(), Cout, out.data_ptr(), stream(dev)))


def first_conv_workspace_bytes(images, Cout):
    """ssd_first_conv_train_workspace_bytes: images is the batch or its (B, H, W)."""
    return lib().ssd_first_conv_train_workspace_bytes(*tuple(getattr(images, "shape", images))[:3], Cout)


def first_conv_backward(images, dy, dw, workspace=None):
    """ssd_first_conv_train_backward from the images uint8 [B,H,W,3] and dy [B,H/2,W/2,Cout]: dw [3,3,3,Cout]."""
    B, H, W, _ = _dense(images, "images", (None, None, None, 3), torch.uint8)
    Cout = _dense(dy, "dy", (B, H // 2, W // 2, None))[3]
    _dense(dw, "dw", (3, 3, 3, Cout))
    dev = _one_gpu(workspace, images=images, dy=dy, dw=dw)
    L = lib()
    _run(dev, workspace, lambda: L.ssd_first_conv_train_workspace_bytes(B, H, W, Cout),
         lambda *tail: L.ssd_first_conv_train_backward(images.data_ptr(), dy.data_ptr(), B, H, W, Cout, dw.data_ptr(), *tail))


def first_conv_f32_forward(images, kernel, out):
    """ssd_first_conv_f32_train_forward: images float32 [B,H,W,3] in [0, 1], kernel [3,3,3,Cout] -> out [B,H/2,W/2,Cout]."""
    B, H, W, _ = _dense(images, "images", (None, None, None, 3), torch.float32)
    Cout = _dense(kernel, "kernel", (3, 3, 3, None))[3]
    _dense(out, "out", (B, H // 2, W // 2, Cout))
    dev = _one_gpu(None, images=images, kernel=kernel, out=out)
    with torch.cuda.device(dev):
        check(lib().ssd_first_conv_f32_train_forward(images.data_ptr(), B, H, W, kernel.data_ptr(), Cout, out.data_ptr(), stream(dev)))


def first_conv_f32_workspace_bytes(images, Cout):
    """ssd_first_conv_f32_train_workspace_bytes: images is the batch or its (B, H, W)."""
    return lib().ssd_first_conv_f32_train_workspace_bytes(*tuple(getattr(images, "shape", images))[:3], Cout)


def first_conv_f32_backward(images, dy, dw, workspace=None):
    """ssd_first_conv_f32_train_backward from the images float32 [B,H,W,3] and dy [B,H/2,W/2,Cout]: dw [3,3,3,Cout]."""
    B, H, W, _ = _dense(images, "images", (None, None, None, 3), torch.float32)
    Cout = _dense(dy, "dy", (B, H // 2, W // 2, None))[3]
    _dense(dw, "dw", (3, 3, 3, Cout))
    dev = _one_gpu(workspace, images=images, dy=dy, dw=dw)
    L = lib()
    _run(dev, workspace, lambda: L.ssd_first_conv_f32_train_workspace_bytes(B, H, W, Cout),
         lambda *tail: L.ssd_first_conv_f32_train_backward(images.data_ptr(), dy.data_ptr(), B, H, W, Cout, dw.data_ptr(), *tail))


# ----------------------------------------------------------------------------- the batch norm
def bn_workspace_bytes(rows, C):
    """ssd_bn_relu_train_workspace_bytes (it sizes both families): rows are row counts or [..., C] tensors."""
    rows = [r.numel() // C if isinstance(r, torch.Tensor) else r for r in rows]
    return lib().ssd_bn_relu_train_workspace_bytes((SsdBnLevel * len(rows))(*[SsdBnLevel(r) for r in rows]), len(rows), C)


def _bn_call(which, entry, act, scalars, workspace, xs, dys, outs, out_name, **vectors):
    """Both batch-norm calls: xs, dys, outs [..., C] of equal shape per level, every column of `vectors` (named after ssd_bn_level's
    fields) None or one per-channel vector per level; <family><which>(levels, n, C[, act], *scalars, workspace, stream)."""
    if entry not in ("bn_act", "bn_relu", "sn_bn") or act not in (SN_ACTS if entry == "sn_bn" else ACTS) or (entry == "bn_relu" and act != "relu"):
        raise ValueError("entry must be 'bn_act', 'bn_relu' (act 'relu' only) or 'sn_bn' (act 'none' too), act 'relu' or 'relu6'")
    xs = _levels(xs)
    n, C, shapes = len(xs), xs[0].shape[-1] if isinstance(xs[0], torch.Tensor) and xs[0].dim() else 0, []
    for i, x in enumerate(xs):
        if not (C and isinstance(x, torch.Tensor)):
            raise ValueError("xs[%d] must be a tensor [..., C]" % i)
        shapes.append(_dense(x, "xs[%d]" % i, (None,) * (x.dim() - 1) + (C,)))
    dys, outs = _column(dys, "dys", shapes), _column(outs, out_name, shapes)
    lv = (SsdBnLevel * n)()
    for i, x in enumerate(xs):
        lv[i].rows = x.numel() // C
        lv[i].x, lv[i].dy, lv[i].out = x.data_ptr(), dys[i].data_ptr() if dys is not None else None, outs[i].data_ptr()
    for name, col in vectors.items():
        if col is not None:
            if len(col) != n:
                raise ValueError("%ss: one vector for every one of the %d levels" % (name, n))
            for i, t in enumerate(col):
                setattr(lv[i], name, _vector(t, "%ss[%d]" % (name, i), C))
    dev = _one_gpu(workspace, xs=xs, dys=dys, **{out_name: outs}, **vectors)
    fn, acts = getattr(lib(), "ssd_%s_train_%s" % (entry, which)), (SN_ACTS[act],) if entry != "bn_relu" else ()
    _run(dev, workspace, lambda: lib().ssd_bn_relu_train_workspace_bytes(lv, n, C), lambda *tail: fn(lv, n, C, *acts, *scalars, *tail))


def bn_forward(xs, outs, gammas, betas, training, epsilon, one_minus_momentum, moving_means=None, moving_variances=None, means=None,
               vars_=None, invstds=None, act="relu", workspace=None, entry="bn_act"):
    """ssd_bn_act_train_forward (entry "bn_relu": ssd_bn_relu_train_forward, act "relu"; "sn_bn": ssd_sn_bn_train_forward, act "none"
    too) of the levels xs [..., C] into outs; every
    other argument a list of [C] vectors per level.  training: the batch statistics go to means, vars_ (nullable), invstds and move
    the moving statistics (nullable as a pair); not training: the inference form on the moving statistics, nothing else written."""
    _bn_call("forward", entry, act, (1 if training else 0, epsilon, one_minus_momentum), workspace, xs, None, outs, "outs", gamma=gammas, beta=betas,
             moving_mean=moving_means, moving_variance=moving_variances, mean=means, var=vars_, invstd=invstds)


def bn_backward(xs, dys, dxs, gammas, betas, means, invstds, dgammas, dbetas, act="relu", workspace=None, entry="bn_act"):
    """ssd_bn_act_train_backward (entry "bn_relu": ssd_bn_relu_train_backward, act "relu"; "sn_bn": ssd_sn_bn_train_backward, act "none"
    too) from xs, dys and the forward's means and
    invstds: dxs of the levels' shapes, dgammas and dbetas [C] per level."""
    _bn_call("backward", entry, act, (), workspace, xs, dys, dxs, "dxs", gamma=gammas, beta=betas, mean=means, invstd=invstds, dgamma=dgammas,
             dbeta=dbetas)


# ----------------------------------------------------------------------------- the TRAIN ShuffleNet's copies and its max pool
def _halves(x, y, xname, yname):
    """x and y [..., D] of one shape -> (rows, D)."""
    if not (isinstance(x, torch.Tensor) and x.dim() >= 1 and x.shape[-1] >= 1):
        raise ValueError("%s must be a tensor [..., D]" % xname)
    shape = _dense(x, xname, (None,) * x.dim())
    _dense(y, yname, tuple(shape))
    return x.numel() // shape[-1], shape[-1]


def shuffle(x, y, xo, yo, transpose=False):
    """ssd_sn_shuffle_train on four tensors [..., D] of one shape: concat_shuffle_split(x, y) -> (xo, yo); transpose: x, y are the
    gradients of the two outputs and xo, yo receive those of the two inputs."""
    rows, D = _halves(x, y, "x", "y")
    _dense(xo, "xo", tuple(x.shape))
    _dense(yo, "yo", tuple(x.shape))
    dev = _one_gpu(None, x=x, y=y, xo=xo, yo=yo)
    with torch.cuda.device(dev):
        check(lib().ssd_sn_shuffle_train(x.data_ptr(), y.data_ptr(), rows, D, 1 if transpose else 0, xo.data_ptr(), yo.data_ptr(), stream(dev)))


def concat(x, y, out):
    """ssd_sn_concat_train: x, y [..., D] -> out [..., 2D] = [x | y]."""
    rows, D = _halves(x, y, "x", "y")
    _dense(out, "out", tuple(x.shape[:-1]) + (2 * D,))
    dev = _one_gpu(None, x=x, y=y, out=out)
    with torch.cuda.device(dev):
        check(lib().ssd_sn_concat_train(x.data_ptr(), y.data_ptr(), rows, D, out.data_ptr(), stream(dev)))


def split(g, dx, dy):
    """ssd_sn_split_train: g [..., 2D] -> dx = g[..., :D], dy = g[..., D:]."""
    rows, D = _halves(dx, dy, "dx", "dy")
    _dense(g, "g", tuple(dx.shape[:-1]) + (2 * D,))
    dev = _one_gpu(None, g=g, dx=dx, dy=dy)
    with torch.cuda.device(dev):
        check(lib().ssd_sn_split_train(g.data_ptr(), rows, D, dx.data_ptr(), dy.data_ptr(), stream(dev)))


def maxpool_backward(x, dy, dx):
    """ssd_sn_maxpool_train_backward: x [B,H,W,C] (the pool's input), dy [B,H/2,W/2,C] -> dx of x's shape."""
    B, H, W, C = _dense(x, "x", (None,) * 4)
    _dense(dy, "dy", (B, H // 2, W // 2, C))
    _dense(dx, "dx", (B, H, W, C))
    dev = _one_gpu(None, x=x, dy=dy, dx=dx)
    with torch.cuda.device(dev):
        check(lib().ssd_sn_maxpool_train_backward(x.data_ptr(), dy.data_ptr(), B, H, W, C, dx.data_ptr(), stream(dev)))


# ----------------------------------------------------------------------------- the TRAIN step's norms
ROW_BYTES = 56                                                                 # sizeof(ssd_update_tensor)


def _rows_host(rows_host, T):
    """rows_host is the host copy of the update's table: a contiguous CPU uint8 tensor of exactly T * 56 bytes -> T."""
    if not (isinstance(rows_host, torch.Tensor) and rows_host.dtype == torch.uint8 and not rows_host.is_cuda and rows_host.dim() == 1
            and rows_host.is_contiguous() and rows_host.numel() % ROW_BYTES == 0 and rows_host.numel() >= ROW_BYTES):
        raise ValueError("rows_host must be a contiguous 1-D uint8 CPU tensor of T * %d bytes (ssd_update_tensor rows)" % ROW_BYTES)
    if T is not None and rows_host.numel() != T * ROW_BYTES:
        raise ValueError("rows_host must hold exactly T = %d rows of %d bytes" % (T, ROW_BYTES))
    return rows_host.numel() // ROW_BYTES


def train_norms_workspace_bytes(rows_host, T=None):
    """ssd_train_norms_workspace_bytes of the table's host copy (0: a table of empty tensors, or one the call would refuse)."""
    T = _rows_host(rows_host, T)
    return lib().ssd_train_norms_workspace_bytes(rows_host.data_ptr(), T)


def train_norms(rows_host, rows_dev, sums, bad, workspace=None):
    """ssd_train_norms over the update's table: rows_host (CPU uint8, T * 56 bytes) is checked, rows_dev (the same bytes on the GPU,
    the caller's upload, ordered before this call on the current stream) is what the kernels read; sums float64 [T,2] receives
    sum w^2, sum g^2 and bad int64 [T,2] the non-finite counts, rows in table order."""
    T = _rows_host(rows_host, None)
    _dense(rows_dev, "rows_dev", (T * ROW_BYTES,), torch.uint8)
    _dense(sums, "sums", (T, 2), torch.float64)
    _dense(bad, "bad", (T, 2), torch.int64)
    dev = _one_gpu(workspace, rows_dev=rows_dev, sums=sums, bad=bad)
    L = lib()
    _run(dev, workspace, lambda: L.ssd_train_norms_workspace_bytes(rows_host.data_ptr(), T),
         lambda *tail: L.ssd_train_norms(rows_host.data_ptr(), rows_dev.data_ptr(), T, sums.data_ptr(), bad.data_ptr(), *tail))


# ----------------------------------------------------------------------------- the TRAIN step's histograms
STATS_BYTES = 40                                                               # sizeof(ssd_histogram_stats)
# ssd_histogram_stats of include/ssd_hip.h: what a host copy of `stats` (uint8 [T,2,40]) is viewed as
STATS_DTYPE = np.dtype([("sum", "<f8"), ("sum_squares", "<f8"), ("min", "<f4"), ("max", "<f4"), ("num", "<i8"), ("bad", "<i8")])
assert STATS_DTYPE.itemsize == STATS_BYTES
_limits = None


def histogram_limits():
    """ssd_histogram_limits: TF's default histogram limits as a read-only numpy float64 table [NB] (the library's ONE definition)."""
    global _limits
    if _limits is None:
        L = lib()
        NB = L.ssd_histogram_limits(None, 0)
        out = np.empty(NB, np.float64)
        if L.ssd_histogram_limits(out.ctypes.data, NB) != NB:
            raise RuntimeError("ssd_histogram_limits changed its answer")
        out.setflags(write=False)
        _limits = out
    return _limits


def train_histograms_workspace_bytes(rows_host, T=None):
    """ssd_train_histograms_workspace_bytes of the table's host copy (0: a table of empty tensors, or one the call would refuse)."""
    T = _rows_host(rows_host, T)
    return lib().ssd_train_histograms_workspace_bytes(rows_host.data_ptr(), T)


def train_histograms(rows_host, rows_dev, weight_decay, limits_dev, counts, stats, workspace=None):
    """ssd_train_histograms over the update's table (rows_host, rows_dev as for train_norms): limits_dev is histogram_limits() on the
    GPU (float64 [NB], the caller's one upload), counts int64 [T,2,NB] receives the bucket counts of w and of the gradient of
    total_loss (g + weight_decay * w on decaying rows), stats uint8 [T,2,40] the ssd_histogram_stats (STATS_DTYPE on the host)."""
    T = _rows_host(rows_host, None)
    NB = len(histogram_limits())
    _dense(rows_dev, "rows_dev", (T * ROW_BYTES,), torch.uint8)
    _dense(limits_dev, "limits_dev", (NB,), torch.float64)
    _dense(counts, "counts", (T, 2, NB), torch.int64)
    _dense(stats, "stats", (T, 2, STATS_BYTES), torch.uint8)
    dev = _one_gpu(workspace, rows_dev=rows_dev, limits_dev=limits_dev, counts=counts, stats=stats)
    L = lib()
    wd = ctypes.c_float(float(weight_decay))
    _run(dev, workspace, lambda: L.ssd_train_histograms_workspace_bytes(rows_host.data_ptr(), T),
         lambda *tail: L.ssd_train_histograms(rows_host.data_ptr(), rows_dev.data_ptr(), T, wd, limits_dev.data_ptr(), counts.data_ptr(),
                                              stats.data_ptr(), *tail))


# ----------------------------------------------------------------------------- the per-level top losses
LOSS_MAX_LEVELS = 8                                                            # SSD_LOSS_MAX_LEVELS
LOSS_TOP_MAX_K = 32768                                                         # SSD_LOSS_TOP_MAX_K


def _level_array(anchors_per_level):
    """anchors_per_level as the int64 array the entry points read (any length: the library refuses what it does not take)."""
    try:
        levels = [int(n) for n in anchors_per_level]
    except TypeError:
        raise ValueError("anchors_per_level must be a sequence of integers") from None
    return (ctypes.c_int64 * max(len(levels), 1))(*levels), len(levels)


def loss_top_counts(anchors_per_level):
    """ssd_loss_top_counts: the per-level counts k_l = ceil(n_l / 5) as a tuple (their sum is K); SsdError for levels the family
    refuses."""
    arr, L = _level_array(anchors_per_level)
    out = (ctypes.c_int64 * max(L, 1))()
    K = lib().ssd_loss_top_counts(arr, L, out)
    if K < 0:
        check(-1)
    counts = tuple(int(out[l]) for l in range(L))
    assert sum(counts) == K
    return counts


def loss_top_workspace_bytes(B, anchors_per_level):
    """ssd_loss_top_workspace_bytes: 2 * B * K floats (0: a call that would be refused)."""
    arr, L = _level_array(anchors_per_level)
    return lib().ssd_loss_top_workspace_bytes(int(B), arr, L)


def loss_top_means(cls_losses, loc_losses, anchors_per_level, means, workspace=None):
    """ssd_loss_top_means: cls_losses and loc_losses float32 [B,N] (ssd_loss's per-anchor planes), anchors_per_level summing to N;
    means float32 [2,K] (K = sum(loss_top_counts(anchors_per_level))) receives the mean over the batch of every image's j-th
    largest loss of each level, plane 0 the classification, plane 1 the localisation losses."""
    B, N = _dense(cls_losses, "cls_losses", (None, None))
    _dense(loc_losses, "loc_losses", (B, N))
    arr, L = _level_array(anchors_per_level)
    _dense(means, "means", (2, sum(loss_top_counts(anchors_per_level))))
    dev = _one_gpu(workspace, cls_losses=cls_losses, loc_losses=loc_losses, means=means)
    fn = lib().ssd_loss_top_means
    _run(dev, workspace, lambda: lib().ssd_loss_top_workspace_bytes(B, arr, L),
         lambda *tail: fn(cls_losses.data_ptr(), loc_losses.data_ptr(), B, N, arr, L, means.data_ptr(), *tail))


# ----------------------------------------------------------------------------- the TRAIN step's gradient exchange
REDUCE_ROW_BYTES = 32                                                          # sizeof(ssd_reduce_row)
REDUCE_HEADER_FLOATS = 16                                                      # SSD_REDUCE_HEADER_FLOATS
REDUCE_MAX_RANKS = 16                                                          # SSD_REDUCE_MAX_RANKS
REDUCE_BLOCK_ELEMS = 4096                                                      # SSD_UPDATE_BLOCK_ELEMS
# ssd_reduce_row of include/ssd_hip.h
REDUCE_ROW_DTYPE = np.dtype([("data", "<u8"), ("count", "<i8"), ("offset", "<i8"), ("kind", "<i4"), ("reserved", "<i4")])
assert REDUCE_ROW_DTYPE.itemsize == REDUCE_ROW_BYTES


def bucket_layout(counts):
    """The bucket layout of include/ssd_hip.h from the rows' counts alone -> (offsets int64 [T], slice_floats): row t starts at
    offsets[t] = the counts before it, each rounded up to 4; a slice is the 16 header floats and the payload, rounded up to 4096."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    if len(counts) < 1 or (counts < 0).any():
        raise ValueError("counts: at least one row, none negative")
    padded = (counts + 3) // 4 * 4
    ends = np.cumsum(padded)
    payload = (int(ends[-1]) + REDUCE_BLOCK_ELEMS - 1) // REDUCE_BLOCK_ELEMS * REDUCE_BLOCK_ELEMS
    return ends - padded, REDUCE_HEADER_FLOATS + payload


def _reduce_rows_host(rows_host):
    """rows_host is the host copy of the exchange's table: a contiguous CPU uint8 tensor of T * 32 bytes -> T."""
    if not (isinstance(rows_host, torch.Tensor) and rows_host.dtype == torch.uint8 and not rows_host.is_cuda and rows_host.dim() == 1
            and rows_host.is_contiguous() and rows_host.numel() % REDUCE_ROW_BYTES == 0 and rows_host.numel() >= REDUCE_ROW_BYTES):
        raise ValueError("rows_host must be a contiguous 1-D uint8 CPU tensor of T * %d bytes (ssd_reduce_row rows)" % REDUCE_ROW_BYTES)
    return rows_host.numel() // REDUCE_ROW_BYTES


def train_bucket_floats(rows_host):
    """ssd_train_bucket_floats of the table's host copy: the floats of one rank's slice (0: a table the calls would refuse)."""
    T = _reduce_rows_host(rows_host)
    return int(lib().ssd_train_bucket_floats(rows_host.data_ptr(), T))


def train_grad_pack(rows_host, rows_dev, header, slice_):
    """ssd_train_grad_pack: rows_host (CPU uint8, T * 32 bytes) is checked, rows_dev (the same bytes on the GPU, the caller's upload,
    ordered before this call on the current stream) is what the kernel reads; header float32 [3] (matches, localization loss,
    classification loss) on the GPU; slice_ float32 [16 + P] receives every float of this rank's slice."""
    T = _reduce_rows_host(rows_host)
    _dense(rows_dev, "rows_dev", (T * REDUCE_ROW_BYTES,), torch.uint8)
    _dense(header, "header", (3,))
    _dense(slice_, "slice_", (None,))
    dev = _one_gpu(None, rows_dev=rows_dev, header=header, slice_=slice_)
    with torch.cuda.device(dev):
        check(lib().ssd_train_grad_pack(rows_host.data_ptr(), rows_dev.data_ptr(), T, header.data_ptr(), slice_.data_ptr(), slice_.numel(),
                                        stream(dev)))


def train_grad_reduce(rows_host, rows_dev, gathered, losses_out, weights_out):
    """ssd_train_grad_reduce: gathered float32 [G, 16 + P] (every rank's slice, rank order) is summed in ascending rank order into
    the rows' tensors; losses_out float32 [2] receives the two losses over the global batch, weights_out float32 [G] the c_r."""
    T = _reduce_rows_host(rows_host)
    _dense(rows_dev, "rows_dev", (T * REDUCE_ROW_BYTES,), torch.uint8)
    G = _dense(gathered, "gathered", (None, None))[0]
    _dense(losses_out, "losses_out", (2,))
    _dense(weights_out, "weights_out", (G,))
    dev = _one_gpu(None, rows_dev=rows_dev, gathered=gathered, losses_out=losses_out, weights_out=weights_out)
    with torch.cuda.device(dev):
        check(lib().ssd_train_grad_reduce(rows_host.data_ptr(), rows_dev.data_ptr(), T, gathered.data_ptr(), G, gathered.shape[1],
                                          losses_out.data_ptr(), weights_out.data_ptr(), stream(dev)))
