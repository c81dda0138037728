"""The trainable FPN on a frozen backbone: detector/feature_extractor.py's fpn() in TRAIN mode on this project's own kernels
(include/ssd_hip.h, "the TRAIN FPN").

    TrainPipeline -> Engine (frozen backbone, retained c3, c4, c5) -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss
                  -> backward (HIP) -> TrainStep over both modules' variables -> checkpoint -> Detector / evaluation

This is the reference's own recipe (train.py:44-50 warm-starts only the backbone; fpn/*, box_net/* and class_net/* start from
their initialisers and are trained), except that the backbone stays frozen: no gradient flows into c3, c4, c5.
conv_same is a torch.autograd.Function over ssd_conv_train_forward / _backward; the FPN's graph is ONE Function whose backward
runs the gradients in a fixed order with ssd_fpn_merge_backward doing every sum, so torch provides memory, streams and the
autograd graph only.  Workspace, stream and level helpers are head_train's.
"""
import ctypes
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._lib import check, lib
from .head_train import _conv_levels, _need, _stream, _workspace, batch_norm_relu

FPN_DEPTH = 256                 # detector/feature_extractor.py:7
LEVELS = (3, 4, 5, 6, 7)


def _out_hw(x, stride):
    return -(-x.shape[1] // stride), -(-x.shape[2] // stride)


def _conv_forward(xs, kernel, bias, stride, ups):
    """ssd_conv_train_forward on contiguous levels -> the outputs."""
    k, Cin, Cout = kernel.shape[0], kernel.shape[2], kernel.shape[3]
    B, dev = xs[0].shape[0], kernel.device
    outs = tuple(torch.empty((B,) + _out_hw(x, stride) + (Cout,), dtype=torch.float32, device=dev) for x in xs)
    lv = _conv_levels(xs, None, outs)
    up = (ctypes.c_void_p * len(xs))(*[u.data_ptr() for u in ups]) if ups is not None else None
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.ssd_conv_train_workspace_bytes(lv, len(xs), B, Cin, Cout, k, stride, 1 if ups is not None else 0))
        check(L.ssd_conv_train_forward(lv, len(xs), B, Cin, Cout, k, stride, kernel.data_ptr(), bias.data_ptr() if bias is not None else None,
                                       up, ws.data_ptr(), ws.numel(), _stream(dev)))
    return outs


def _conv_backward(xs, kernel, dys, stride, want_dx, want_dbias=False):
    """ssd_conv_train_backward -> (dw, dbias or None, dxs or None)."""
    k, Cin, Cout = kernel.shape[0], kernel.shape[2], kernel.shape[3]
    B, dev = xs[0].shape[0], kernel.device
    dxs = tuple(torch.empty_like(x) for x in xs) if want_dx else None
    dw = torch.empty_like(kernel)
    dbias = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dbias else None
    lv = _conv_levels(xs, dys, dxs)
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.ssd_conv_train_workspace_bytes(lv, len(xs), B, Cin, Cout, k, stride, 0))
        check(L.ssd_conv_train_backward(lv, len(xs), B, Cin, Cout, k, stride, kernel.data_ptr(), dw.data_ptr(),
                                        dbias.data_ptr() if dbias is not None else None, ws.data_ptr(), ws.numel(), _stream(dev)))
    return dw, dbias, dxs


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
                                           out.data_ptr(), _stream(g.device)))
    return out


def _zeros_like_out(x, Cout, stride):
    return torch.zeros((x.shape[0],) + _out_hw(x, stride) + (Cout,), dtype=torch.float32, device=x.device)


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kernel, bias, stride, n, *t):
        xs = tuple(x.contiguous() for x in t[:n])
        ups = tuple(u.contiguous() for u in t[n:]) if len(t) > n else None
        kernel = kernel.contiguous()
        outs = _conv_forward(xs, kernel, bias, stride, ups)
        ctx.save_for_backward(kernel, *xs)
        ctx.stride, ctx.n, ctx.has_bias, ctx.has_up = stride, n, bias is not None, ups is not None
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        kernel, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        n, Cout = ctx.n, kernel.shape[3]
        dys = tuple(_zeros_like_out(x, Cout, ctx.stride) if d is None else d.contiguous() for x, d in zip(xs, dys))
        want_dx = any(ctx.needs_input_grad[4:4 + n])
        if want_dx and kernel.shape[0] == 1:
            raise RuntimeError("conv_same: a 1x1 convolution has no data gradient here (nothing trainable lies upstream of a lateral "
                               "while the backbone is frozen); detach its input")
        dw, dbias, dxs = _conv_backward(xs, kernel, dys, ctx.stride, want_dx, ctx.has_bias)
        dups = ()
        if ctx.has_up:                                                  # the gradient of `up`: the 2x2 sums of dy
            dups = tuple(fpn_merge_backward(d) if need else None for d, need in zip(dys, ctx.needs_input_grad[4 + n:]))
        return (dw, dbias, None, None) + (dxs if want_dx else (None,) * n) + dups


def conv_same(features, kernel, stride=1, up=None, bias=None):
    """conv2d_same (layer_utils.py:15-43) of every level with ONE kernel: features a tensor [B,H,W,Cin] or a list of them, kernel
    HWIO [k,k,Cin,Cout] with k = 1 or 3, stride 1 or 2 (2 only with k = 3: the output is ceil(H/2) x ceil(W/2), an explicit pad of 1),
    up (stride 1, even H and W only) a tensor [B,H/2,W/2,Cout] per level that is added after nearest x2 upsampling.  All float32
    CUDA tensors; returns the same kind as `features`.  The forward is bit-identical to ssd_amd.ssd.conv2d with the same arguments
    (mode "EXPLICIT" for stride 2).  Gradients flow to the kernel, the bias, `up` (the 2x2 sums of the output's gradient) and, for
    k = 3, to the features; a 1x1 convolution whose input requires a gradient raises in backward."""
    single = isinstance(features, torch.Tensor)
    xs = [features] if single else list(features)
    if not xs or len(xs) > 8:
        raise ValueError("conv_same takes 1 .. 8 levels")
    _need(kernel, "kernel")
    if kernel.dim() != 4 or kernel.shape[0] != kernel.shape[1] or kernel.shape[0] not in (1, 3):
        raise ValueError("kernel must be HWIO [k,k,Cin,Cout] with k = 1 or 3")
    if stride not in (1, 2) or (stride == 2 and kernel.shape[0] != 3):
        raise ValueError("stride must be 1 or 2, and 2 only with k = 3")
    if bias is not None:
        _need(bias, "bias")
        if tuple(bias.shape) != (kernel.shape[3],):
            raise ValueError("bias must have shape [Cout]")
    for x in xs:
        _need(x, "features")
        if x.dim() != 4 or x.shape[3] != kernel.shape[2] or x.shape[0] != xs[0].shape[0]:
            raise ValueError("every level must be [B,H,W,Cin] with the kernel's Cin and one batch size")
    ups = []
    if up is not None:
        ups = [up] if isinstance(up, torch.Tensor) else list(up)
        if stride != 1 or bias is not None or len(ups) != len(xs):
            raise ValueError("up: one tensor per level, only with stride 1 and without a bias")
        for x, u in zip(xs, ups):
            _need(u, "up")
            if (x.shape[1] | x.shape[2]) & 1 or tuple(u.shape) != (x.shape[0], x.shape[1] // 2, x.shape[2] // 2, kernel.shape[3]):
                raise ValueError("up must be [B,H/2,W/2,Cout] of a level with even H and W")
    outs = _Conv.apply(kernel, bias, stride, len(xs), *(xs + ups))
    return outs[0] if single else list(outs)


class _FpnGraph(torch.autograd.Function):
    """fpn() before its batch norms (feature_extractor.py:57-69) as one node: (c3, c4, c5, the ten kernels) -> raw p3 .. p7.  The
    backward is the fixed sequence of DESIGN.md 4.12; c3, c4, c5 receive no gradient (the backbone is frozen)."""

    @staticmethod
    def forward(ctx, c3, c4, c5, l3, l4, l5, k3, k4, k5, k6, k7):
        c3, c4, c5 = c3.contiguous(), c4.contiguous(), c5.contiguous()
        ks = tuple(k.contiguous() for k in (l3, l4, l5, k3, k4, k5, k6, k7))
        l3, l4, l5, k3, k4, k5, k6, k7 = ks
        x5, = _conv_forward((c5,), l5, None, 1, None)
        p5, = _conv_forward((x5,), k5, None, 1, None)
        p6, = _conv_forward((c5,), k6, None, 2, None)
        r6 = fpn_merge_backward(p6, gate=p6, same_size=True)            # relu(p6): +0 + (p6 > 0 ? p6 : +0)
        p7, = _conv_forward((r6,), k7, None, 2, None)
        x4, = _conv_forward((c4,), l4, None, 1, (x5,))
        p4, = _conv_forward((x4,), k4, None, 1, None)
        x3, = _conv_forward((c3,), l3, None, 1, (x4,))
        p3, = _conv_forward((x3,), k3, None, 1, None)
        ctx.save_for_backward(c3, c4, c5, x3, x4, x5, p6, r6, *ks)
        ctx.shape7 = tuple(p7.shape)
        return p3, p4, p5, p6, p7

    @staticmethod
    @once_differentiable
    def backward(ctx, d3, d4, d5, d6, d7):
        c3, c4, c5, x3, x4, x5, p6, r6, l3, l4, l5, k3, k4, k5, k6, k7 = ctx.saved_tensors
        z = lambda d, like: torch.zeros_like(like) if d is None else d.contiguous()
        d3, d4, d5, d6 = z(d3, x3), z(d4, x4), z(d5, x5), z(d6, p6)
        d7 = torch.zeros(ctx.shape7, dtype=torch.float32, device=r6.device) if d7 is None else d7.contiguous()
        g7, _, (dr6,) = _conv_backward((r6,), k7, (d7,), 2, True)
        dp6 = fpn_merge_backward(dr6, base=d6, gate=p6, same_size=True)  # d p6 (raw) = d p6 from its batch norm + relu'(p6) * d relu(p6)
        g6, _, _ = _conv_backward((c5,), k6, (dp6,), 2, False)
        g3, _, (dx3,) = _conv_backward((x3,), k3, (d3,), 1, True)
        gl3, _, _ = _conv_backward((c3,), l3, (dx3,), 1, False)
        g4, _, (dx4,) = _conv_backward((x4,), k4, (d4,), 1, True)
        fpn_merge_backward(dx3, base=dx4, out=dx4)                      # d x4 = d x4 from p4 + the 2x2 sums of d x3
        gl4, _, _ = _conv_backward((c4,), l4, (dx4,), 1, False)
        g5, _, (dx5,) = _conv_backward((x5,), k5, (d5,), 1, True)
        fpn_merge_backward(dx4, base=dx5, out=dx5)                      # d x5 = d x5 from p5 + the 2x2 sums of d x4
        gl5, _, _ = _conv_backward((c5,), l5, (dx5,), 1, False)
        return None, None, None, gl3, gl4, gl5, g3, g4, g5, g6, g7


def fpn_variable_shapes(params):
    """The FPN's subset of variables.variable_shapes(params): fpn/*, statistics included."""
    from .variables import variable_shapes
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("fpn/")}


def variance_scaling_draw(rng, shape):
    """tf.variance_scaling_initializer() with its defaults (scale 1, fan-in, truncated normal) for an HWIO kernel: every element
    is drawn from a normal distribution of standard deviation s = sqrt(1 / fan_in) / 0.87962566103423978, fan_in = k * k * Cin,
    and re-drawn while it lies outside [-2 s, 2 s]; the constant is the standard deviation of the unit normal truncated at +-2,
    so the kept values have variance 1 / fan_in.  `rng` is a numpy Generator; the draw order is C order, re-draws appended (this
    library's choice: TF's own random stream is not reproduced)."""
    fan_in = int(np.prod(shape[:-1]))
    s = math.sqrt(1.0 / fan_in) / 0.87962566103423978
    a = rng.normal(0.0, s, shape)
    bad = np.abs(a) > 2.0 * s
    while bad.any():
        a[bad] = rng.normal(0.0, s, int(bad.sum()))
        bad = np.abs(a) > 2.0 * s
    return a.astype(np.float32)


class TrainableFPN(torch.nn.Module):
    """fpn(features, is_training) (feature_extractor.py:40-76) as a torch.nn.Module on the HIP kernels, for a FROZEN backbone.

    params   the model config (backbone, depth_multiplier: config.load_config)
    weights  {reference variable name: float32 array in TF layout}; only fpn/* is read.  A variable that is missing -- train.py's
             warm start, where `weights` holds the backbone only -- is drawn with the reference's initialiser: kernels by
             variance_scaling_draw(numpy default_rng(seed), shape) in variables.variable_shapes order, gamma 1, beta 0,
             moving_mean 0, moving_variance 1.
    forward([c3, c4, c5], NHWC, e.g. from ssd.BackboneFeatures) -> [p3, p4, p5, p6, p7]; p7 = conv(relu(RAW p6)), the batch norms
    come last (:71-74).  No gradient flows into c3, c4, c5.  .train(): batch statistics, the moving statistics move; .eval(): the
    engine's inference form, bit for bit.  named_variables() / statistics() are what TrainStep takes, e.g. together with the head's:
    TrainStep({**fpn.named_variables(), **head.named_variables()}, config, {**fpn.statistics(), **head.statistics()}, layout="tf",
    params=params)."""

    def __init__(self, params, weights, device=None, seed=0):
        super().__init__()
        self.params = dict(params)
        self._names, self._stat_names = [], []
        rng = np.random.default_rng(seed)
        for name, shape in fpn_variable_shapes(params).items():
            a = weights.get(name)
            leaf = name.rsplit("/", 1)[1]
            if a is None:
                a = (variance_scaling_draw(rng, shape) if leaf == "kernel" else
                     np.ones(shape) if leaf in ("gamma", "moving_variance") else np.zeros(shape))
            a = np.ascontiguousarray(a, dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("variable %r has shape %s, expected %s" % (name, a.shape, tuple(shape)))
            t = torch.from_numpy(a.copy())
            if device is not None:
                t = t.to(device)
            attr = name.replace("/", "__")
            if leaf in ("moving_mean", "moving_variance"):
                self.register_buffer(attr, t)
                self._stat_names.append(name)
            else:
                self.register_parameter(attr, torch.nn.Parameter(t))
                self._names.append(name)

    def variable(self, name):
        return getattr(self, name.replace("/", "__"))

    def named_variables(self):
        """{reference name: trainable Parameter} in variable_shapes order (TF layout)."""
        return {n: self.variable(n) for n in self._names}

    def statistics(self):
        """{reference name: moving_mean / moving_variance buffer}."""
        return {n: self.variable(n) for n in self._stat_names}

    def forward(self, features):
        feats = list(features)
        if len(feats) != 3:
            raise ValueError("features: [c3, c4, c5]")
        for f in feats:
            _need(f, "features")
        kernels = [self.variable("fpn/lateral%d/kernel" % i) for i in (3, 4, 5)] + [self.variable("fpn/p%d/kernel" % i) for i in LEVELS]
        raw = _FpnGraph.apply(*[f.detach() for f in feats], *kernels)
        bn = ["fpn/p%d_batch_norm" % i for i in LEVELS]
        return batch_norm_relu(list(raw), *[[self.variable("%s/%s" % (s, leaf)) for s in bn]
                                           for leaf in ("gamma", "beta", "moving_mean", "moving_variance")], training=self.training)
