"""The trainable detection head: detector/box_predictor.py's RetinaNetBoxPredictor in TRAIN mode on this project's own
kernels (include/ssd_hip.h, "the TRAIN head").

    TrainPipeline -> Engine (frozen backbone + FPN, retained p3 .. p7) -> TrainableBoxPredictor -> differentiable_loss
                  -> backward (HIP) -> TrainStep -> checkpoint -> Detector / evaluation

conv3x3_same and batch_norm_relu are torch.autograd.Functions over the C entry points (once differentiable); torch provides
memory, streams and the autograd graph only.  Freezing the backbone and the FPN is a MODE of this project, not parity with the
reference, which runs every batch norm of the graph on batch statistics in TRAIN mode.
"""
import ctypes
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import SsdBnLevel, SsdConvLevel, check, lib

BATCH_NORM_MOMENTUM = 0.993     # detector/constants.py
BATCH_NORM_EPSILON = 1e-3
MIN_LEVEL = 3
NUM_ANCHORS_PER_LOCATION = 6
TOWER_DEPTH = 4

_workspaces = {}


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


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _conv_levels(xs, dys, outs):
    lv = (SsdConvLevel * len(xs))()
    for i, x in enumerate(xs):
        lv[i].H, lv[i].W = x.shape[1], x.shape[2]
        lv[i].x = x.data_ptr()
        lv[i].dy = dys[i].data_ptr() if dys is not None else None
        lv[i].out = outs[i].data_ptr() if outs is not None else None
    return lv


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kernel, bias, *xs):
        xs = tuple(x.contiguous() for x in xs)
        kernel = kernel.contiguous()
        B, Cin, Cout = xs[0].shape[0], kernel.shape[2], kernel.shape[3]
        outs = tuple(torch.empty(x.shape[:3] + (Cout,), dtype=torch.float32, device=x.device) for x in xs)
        lv = _conv_levels(xs, None, outs)
        L = lib()
        with torch.cuda.device(kernel.device):
            nbytes = L.ssd_conv3x3_train_workspace_bytes(lv, len(xs), B, Cin, Cout)
            ws = _workspace(kernel.device, nbytes)
            check(L.ssd_conv3x3_train_forward(lv, len(xs), B, Cin, Cout, kernel.data_ptr(), bias.data_ptr() if bias is not None else None,
                                              ws.data_ptr(), ws.numel(), _stream(kernel.device)))
        ctx.save_for_backward(kernel, *xs)
        ctx.has_bias = bias is not None
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        kernel, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        B, Cin, Cout = xs[0].shape[0], kernel.shape[2], kernel.shape[3]
        dys = tuple(torch.zeros(x.shape[:3] + (Cout,), dtype=torch.float32, device=x.device) if d is None else d.contiguous()
                    for x, d in zip(xs, dys))
        want_dx = any(ctx.needs_input_grad[2:])
        dxs = tuple(torch.empty_like(x) for x in xs) if want_dx else None
        dw = torch.empty_like(kernel)
        dbias = torch.empty(Cout, dtype=torch.float32, device=kernel.device) if ctx.has_bias else None
        lv = _conv_levels(xs, dys, dxs)
        L = lib()
        with torch.cuda.device(kernel.device):
            nbytes = L.ssd_conv3x3_train_workspace_bytes(lv, len(xs), B, Cin, Cout)
            ws = _workspace(kernel.device, nbytes)
            check(L.ssd_conv3x3_train_backward(lv, len(xs), B, Cin, Cout, kernel.data_ptr(), dw.data_ptr(),
                                               dbias.data_ptr() if dbias is not None else None, ws.data_ptr(), ws.numel(),
                                               _stream(kernel.device)))
        return (dw, dbias) + (dxs if want_dx else (None,) * len(xs))


def conv3x3_same(features, kernel, bias=None):
    """3x3 stride-1 'same' convolution of every level with ONE kernel (+ bias): features is a tensor [B,H,W,Cin] or a list of
    them (the pyramid levels), kernel HWIO [3,3,Cin,Cout], all float32 CUDA tensors; returns the same kind.  The forward is
    bit-identical to ssd_amd.ssd.conv2d; gradients flow to the features, the kernel and the bias."""
    single = isinstance(features, torch.Tensor)
    xs = [features] if single else list(features)
    if not xs or len(xs) > 8:
        raise ValueError("conv3x3_same takes 1 .. 8 levels")
    _need(kernel, "kernel")
    if kernel.dim() != 4 or tuple(kernel.shape[:2]) != (3, 3):
        raise ValueError("kernel must be HWIO [3,3,Cin,Cout]")
    if bias is not None:
        _need(bias, "bias")
        if tuple(bias.shape) != (kernel.shape[3],):
            raise ValueError("bias must have shape [Cout]")
    for x in xs:
        _need(x, "features")
        if x.dim() != 4 or x.shape[3] != kernel.shape[2] or x.shape[0] != xs[0].shape[0]:
            raise ValueError("every level must be [B,H,W,Cin] with the kernel's Cin and one batch size")
    outs = _Conv3x3.apply(kernel, bias, *xs)
    return outs[0] if single else list(outs)


def _bn_levels(xs, dys, outs, gammas, betas, mms, mvs, means, vars_, invstds, dgammas, dbetas):
    lv = (SsdBnLevel * len(xs))()
    cols = (("x", xs), ("dy", dys), ("out", outs), ("gamma", gammas), ("beta", betas), ("moving_mean", mms), ("moving_variance", mvs),
            ("mean", means), ("var", vars_), ("invstd", invstds), ("dgamma", dgammas), ("dbeta", dbetas))
    for i, x in enumerate(xs):
        lv[i].rows = x.numel() // x.shape[-1]
        for name, col in cols:
            setattr(lv[i], name, col[i].data_ptr() if col is not None and col[i] is not None else None)
    return lv


def _bn_call(fn, lv, n, C, device, *args):
    L = lib()
    with torch.cuda.device(device):
        ws = _workspace(device, L.ssd_bn_relu_train_workspace_bytes(lv, n, C))
        check(fn(lv, n, C, *args, ws.data_ptr(), ws.numel(), _stream(device)))


class _BnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, epsilon, one_minus_momentum, *t):
        xs = tuple(x.contiguous() for x in t[:n])
        gammas, betas, mms, mvs = t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n], t[4 * n:5 * n]
        C, dev = xs[0].shape[-1], xs[0].device
        outs = tuple(torch.empty_like(x) for x in xs)
        Cp = (C + 3) // 4 * 4                                                  # rows of 16-byte multiples: every vector is aligned for any C
        stats = torch.empty((n, 3, Cp), dtype=torch.float32, device=dev)      # mean, var, invstd per level
        means, vars_, invstds = [stats[i, 0, :C] for i in range(n)], [stats[i, 1, :C] for i in range(n)], [stats[i, 2, :C] for i in range(n)]
        lv = _bn_levels(xs, None, outs, gammas, betas, mms, mvs, means, vars_, invstds, None, None)
        _bn_call(lib().ssd_bn_relu_train_forward, lv, n, C, dev, 1, epsilon, one_minus_momentum)
        ctx.save_for_backward(stats, *(xs + tuple(gammas) + tuple(betas)))
        ctx.n = n
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        n = ctx.n
        stats, t = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        xs, gammas, betas = t[:n], t[n:2 * n], t[2 * n:3 * n]
        C, dev = xs[0].shape[-1], xs[0].device
        dys = tuple(torch.zeros_like(x) if d is None else d.contiguous() for x, d in zip(xs, dys))
        dxs = tuple(torch.empty_like(x) for x in xs)
        grads = torch.empty((n, 2, (C + 3) // 4 * 4), dtype=torch.float32, device=dev)
        dgammas, dbetas = [grads[i, 0, :C] for i in range(n)], [grads[i, 1, :C] for i in range(n)]
        means, invstds = [stats[i, 0, :C] for i in range(n)], [stats[i, 2, :C] for i in range(n)]
        lv = _bn_levels(xs, dys, dxs, gammas, betas, None, None, means, None, invstds, dgammas, dbetas)
        _bn_call(lib().ssd_bn_relu_train_backward, lv, n, C, dev)
        return (None, None, None) + dxs + tuple(dgammas) + tuple(dbetas) + (None,) * (2 * n)


def batch_norm_relu(x, gamma, beta, moving_mean, moving_variance, training, momentum=BATCH_NORM_MOMENTUM, epsilon=BATCH_NORM_EPSILON):
    """layer_utils.py:5-12: batch norm + ReLU of x [..., C] with its own gamma, beta and moving statistics [C] -- or of a LIST of
    levels, each argument then a list (one launch sequence for all of them).  training=True: the batch's statistics (biased
    variance), the moving statistics are updated in place (moving -= (moving - batch) * (1 - momentum), unbiased variance);
    gradients flow to x, gamma and beta.  training=False: the inference form (x - moving_mean) * sf + beta that the engine
    folds into its convolutions, bit for bit; no gradient."""
    single = isinstance(x, torch.Tensor)
    cols = [[v] if single else list(v) for v in (x, gamma, beta, moving_mean, moving_variance)]
    n = len(cols[0])
    if n < 1 or n > 8 or any(len(c) != n for c in cols):
        raise ValueError("batch_norm_relu takes 1 .. 8 levels, every argument one entry per level")
    C = cols[0][0].shape[-1]
    for i in range(n):
        for c, name in zip(cols, ("x", "gamma", "beta", "moving_mean", "moving_variance")):
            _need(c[i], name)
            if c[i].shape[-1] != C or (name != "x" and c[i].dim() != 1) or not (name == "x" or c[i].is_contiguous()):
                raise ValueError("%s of level %d: contiguous, %d channels" % (name, i, C))
    eps = float(np.float32(epsilon))
    if training:
        omm = float(np.float32(1.0 - momentum))
        outs = _BnRelu.apply(n, eps, omm, *(cols[0] + cols[1] + cols[2] + cols[3] + cols[4]))
    else:
        xs = [v.detach().contiguous() for v in cols[0]]
        outs = [torch.empty_like(v) for v in xs]
        lv = _bn_levels(xs, None, outs, cols[1], cols[2], cols[3], cols[4], None, None, None, None, None)
        _bn_call(lib().ssd_bn_relu_train_forward, lv, n, C, xs[0].device, 0, eps, 0.0)
    return outs[0] if single else list(outs)


def head_variable_shapes(params):
    """The head's subset of variables.variable_shapes(params): box_net/* and class_net/*, statistics included."""
    from .variables import variable_shapes
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("box_net/") or k.startswith("class_net/")}


class TrainableBoxPredictor(torch.nn.Module):
    """RetinaNetBoxPredictor(is_training, num_classes) (box_predictor.py:34-155) as a torch.nn.Module on the HIP kernels.

    params   the model config (num_classes, backbone, depth_multiplier: config.load_config)
    weights  {reference variable name: float32 array in TF layout}, e.g. load_ckpt_weights / synthetic_weights output; only
             box_net/* and class_net/* are read.  A `class_net/logits` whose width is not 6 * num_classes (a new class list) is
             re-drawn with the reference's initialiser: normal(0, 0.01) from `seed`, bias -log(99).
    forward([p3 .. p7], NHWC) -> encoded_boxes [B,N,4], class_predictions [B,N,num_classes] in the anchor order of
    reshape_and_concatenate (:67-104).  .train(): batch statistics, moving statistics move; .eval(): the engine's inference form.
    named_variables() / statistics() are what TrainStep(named_variables(), config, statistics(), layout="tf", params=params) takes."""

    def __init__(self, params, weights, device=None, seed=0):
        super().__init__()
        self.params = dict(params)
        self.num_classes = int(params["num_classes"])
        self._names, self._stat_names = [], []
        rng = np.random.default_rng(seed)
        for name, shape in head_variable_shapes(params).items():
            a = weights.get(name)
            if name.startswith("class_net/logits/") and (a is None or tuple(np.shape(a)) != tuple(shape)):
                a = rng.normal(0.0, 0.01, shape) if name.endswith("kernel") else np.full(shape, -math.log(99.0))
            if a is None:
                raise KeyError("weights has no variable %r" % name)
            a = np.ascontiguousarray(a, dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("variable %r has shape %s, expected %s" % (name, a.shape, tuple(shape)))
            t = torch.from_numpy(a.copy())
            if device is not None:
                t = t.to(device)
            attr = name.replace("/", "__")
            if name.rsplit("/", 1)[1] in ("moving_mean", "moving_variance"):
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

    def _net(self, net, last, features):
        n = len(features)
        x = list(features)
        for i in range(TOWER_DEPTH):
            x = conv3x3_same(x, self.variable("%s/conv3x3_%d/kernel" % (net, i)))
            bn = ["%s/batch_norm_%d_for_level_%d" % (net, i, MIN_LEVEL + l) for l in range(n)]
            x = batch_norm_relu(x, *[[self.variable("%s/%s" % (s, leaf)) for s in bn]
                                     for leaf in ("gamma", "beta", "moving_mean", "moving_variance")], training=self.training)
        return conv3x3_same(x, self.variable("%s/%s/kernel" % (net, last)), self.variable("%s/%s/bias" % (net, last)))

    def forward(self, image_features):
        feats = list(image_features)
        if not 1 <= len(feats) <= 5:
            raise ValueError("image_features: the pyramid levels p3 .. (at most five)")
        boxes = self._net("box_net", "encoded_boxes", feats)
        logits = self._net("class_net", "logits", feats)
        B = feats[0].shape[0]
        encoded = torch.cat([y.reshape(B, -1, 4) for y in boxes], dim=1)
        classes = torch.cat([y.reshape(B, -1, self.num_classes) for y in logits], dim=1)
        return encoded, classes
