"""The differentiable ops under the trainable modules (include/ssd_hip.h, "the TRAIN head", "the TRAIN FPN" and "the TRAIN
backbone" and "the TRAIN first convolution"), and nothing about any model: conv_same / conv3x3_same, depthwise_conv, pointwise_conv,
first_conv_train and batch_norm_act (batch_norm_relu is its act="relu" case) are torch.autograd.Functions over the C entry points (once differentiable), fpn_merge_backward is
ssd_fpn_merge_backward, and ReferenceVariables is the torch.nn.Module base that holds a block's variables under their reference
names.  torch provides memory, streams and the autograd graph only.  head_train.py, fpn_train.py and backbone_train.py build
RetinaNetBoxPredictor, fpn() and mobilenet_v1() from these.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._lib import SsdBnLevel, SsdConvLevel, check, lib

BATCH_NORM_MOMENTUM = 0.993     # detector/constants.py
BATCH_NORM_EPSILON = 1e-3

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


# ----------------------------------------------------------------------------- the convolution
def _conv_levels(xs, dys, outs):
    lv = (SsdConvLevel * len(xs))()
    for i, x in enumerate(xs):
        lv[i].H, lv[i].W = x.shape[1], x.shape[2]
        lv[i].x = x.data_ptr()
        lv[i].dy = dys[i].data_ptr() if dys is not None else None
        lv[i].out = outs[i].data_ptr() if outs is not None else None
    return lv


def _out_shape(x, Cout, stride):
    return (x.shape[0], -(-x.shape[1] // stride), -(-x.shape[2] // stride), Cout)


def _conv_forward(xs, kernel, bias, stride, ups):
    """ssd_conv_train_forward on contiguous levels -> the outputs."""
    k, Cin, Cout = kernel.shape[0], kernel.shape[2], kernel.shape[3]
    B, dev = xs[0].shape[0], kernel.device
    outs = tuple(torch.empty(_out_shape(x, Cout, stride), dtype=torch.float32, device=dev) for x in xs)
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


def _pointwise_backward(xs, kernel, dys, want_dx):
    """ssd_pointwise_train_backward -> (dw, dxs or None): _conv_backward's k = 1 call with the data gradient."""
    Cin, Cout = kernel.shape[2], kernel.shape[3]
    B, dev = xs[0].shape[0], kernel.device
    dxs = tuple(torch.empty_like(x) for x in xs) if want_dx else None
    dw = torch.empty_like(kernel)
    lv = _conv_levels(xs, dys, dxs)
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.ssd_pointwise_train_workspace_bytes(lv, len(xs), B, Cin, Cout))
        check(L.ssd_pointwise_train_backward(lv, len(xs), B, Cin, Cout, kernel.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _stream(dev)))
    return dw, dxs


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


class _Conv(torch.autograd.Function):
    """(kernel, bias, stride, n, the n levels, then one `up` per level or none) -> the n outputs."""

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
        dys = tuple(torch.zeros(_out_shape(x, Cout, ctx.stride), dtype=torch.float32, device=x.device) if d is None else d.contiguous()
                    for x, d in zip(xs, dys))
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


def conv3x3_same(features, kernel, bias=None):
    """conv_same for the head: kernel HWIO [3,3,Cin,Cout], stride 1 (+ bias).  The forward is bit-identical to ssd_amd.ssd.conv2d;
    gradients flow to the features, the kernel and the bias."""
    _need(kernel, "kernel")
    if kernel.dim() != 4 or tuple(kernel.shape[:2]) != (3, 3):
        raise ValueError("kernel must be HWIO [3,3,Cin,Cout]")
    return conv_same(features, kernel, bias=bias)


# ----------------------------------------------------------------------------- the backbone's convolutions
class _Pointwise(torch.autograd.Function):
    """(kernel, the n levels) -> the n outputs of the 1x1 convolution; the backward is ssd_pointwise_train_backward."""

    @staticmethod
    def forward(ctx, kernel, *xs):
        xs = tuple(x.contiguous() for x in xs)
        kernel = kernel.contiguous()
        outs = _conv_forward(xs, kernel, None, 1, None)
        ctx.save_for_backward(kernel, *xs)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        kernel, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dys = tuple(torch.zeros(_out_shape(x, kernel.shape[3], 1), dtype=torch.float32, device=x.device) if d is None else d.contiguous()
                    for x, d in zip(xs, dys))
        want_dx = any(ctx.needs_input_grad[1:])
        dw, dxs = _pointwise_backward(xs, kernel, dys, want_dx)
        return (dw,) + (dxs if want_dx else (None,) * len(xs))


def pointwise_conv(features, kernel):
    """slim.conv2d 1x1, stride 1, raw (mobilenet_v1.py:66 before its batch norm): features a tensor [B,H,W,Cin] or a list of them that
    share ONE kernel HWIO [1,1,Cin,Cout], Cin a multiple of 4.  The forward is conv_same's (bit-identical to ssd_amd.ssd.conv2d);
    gradients flow to the kernel AND to the features (dx = conv1x1(dy, kernel transposed), one fmaf chain per element)."""
    single = isinstance(features, torch.Tensor)
    xs = [features] if single else list(features)
    if not xs or len(xs) > 8:
        raise ValueError("pointwise_conv takes 1 .. 8 levels")
    _need(kernel, "kernel")
    if kernel.dim() != 4 or tuple(kernel.shape[:2]) != (1, 1):
        raise ValueError("kernel must be HWIO [1,1,Cin,Cout]")
    for x in xs:
        _need(x, "features")
        if x.dim() != 4 or x.shape[3] != kernel.shape[2] or x.shape[0] != xs[0].shape[0]:
            raise ValueError("every level must be [B,H,W,Cin] with the kernel's Cin and one batch size")
    outs = _Pointwise.apply(kernel, *xs)
    return outs[0] if single else list(outs)


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride):
        x, kernel = x.contiguous(), kernel.contiguous()
        B, H, W, C = x.shape
        out = torch.empty((B, -(-H // stride), -(-W // stride), C), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib().ssd_depthwise_train_forward(x.data_ptr(), B, H, W, C, kernel.data_ptr(), stride, out.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(x, kernel)
        ctx.stride = stride
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, kernel = ctx.saved_tensors
        B, H, W, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(kernel)
        L = lib()
        with torch.cuda.device(x.device):
            ws = _workspace(x.device, L.ssd_depthwise_train_workspace_bytes(B, H, W, C, ctx.stride))
            check(L.ssd_depthwise_train_backward(x.data_ptr(), dy.data_ptr(), B, H, W, C, kernel.data_ptr(), ctx.stride,
                                                 dx.data_ptr() if dx is not None else None, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _stream(x.device)))
        return dx, dw, None


def depthwise_conv(x, kernel, stride=1):
    """tf.nn.depthwise_conv2d, 3x3, 'SAME', raw (depthwise_conv.py:5-26 before its batch norm): x [B,H,W,C], kernel [3,3,C,1], C a
    multiple of 4 (at most 1024 for the backward), stride 1 or 2 (2: H and W of one parity).  The forward is bit-identical to
    ssd_amd.ssd.depthwise3x3 without batch norm and activation; gradients flow to x and the kernel."""
    _need(x, "x")
    _need(kernel, "kernel")
    if x.dim() != 4 or tuple(kernel.shape) != (3, 3, x.shape[3], 1):
        raise ValueError("x must be [B,H,W,C] and kernel [3,3,C,1]")
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2")
    return _Depthwise.apply(x, kernel, stride)


class _FirstConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, kernel):
        images, kernel = images.contiguous(), kernel.contiguous()
        B, H, W, _ = images.shape
        Cout = kernel.shape[3]
        out = torch.empty((B, H // 2, W // 2, Cout), dtype=torch.float32, device=images.device)
        with torch.cuda.device(images.device):
            check(lib().ssd_first_conv_train_forward(images.data_ptr(), B, H, W, kernel.data_ptr(), Cout, out.data_ptr(), _stream(images.device)))
        ctx.save_for_backward(images)
        ctx.Cout = Cout
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        images, = ctx.saved_tensors
        B, H, W, _ = images.shape
        dy = dy.contiguous()
        dw = torch.empty((3, 3, 3, ctx.Cout), dtype=torch.float32, device=images.device)
        L = lib()
        with torch.cuda.device(images.device):
            ws = _workspace(images.device, L.ssd_first_conv_train_workspace_bytes(B, H, W, ctx.Cout))
            check(L.ssd_first_conv_train_backward(images.data_ptr(), dy.data_ptr(), B, H, W, ctx.Cout, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _stream(images.device)))
        return None, dw


def first_conv_train(images, kernel):
    """slim.conv2d 3x3, stride 2, 'SAME', raw, on the normalised frames (mobilenet_v1.py:34-50 before its batch norm): images uint8
    [B,H,W,3] on the GPU at the network's own size (H and W even), kernel [3,3,3,Cout], Cout a multiple of 4 and at most 64.  The
    pixel value is the inference path's 2 * (u / 255) - 1.  The forward is bit-identical to ssd_amd.ssd.first_conv without batch norm
    and activation; the gradient flows to the kernel only (the input is the image)."""
    if not (isinstance(images, torch.Tensor) and images.dtype == torch.uint8):
        raise TypeError("images must be a uint8 tensor on a GPU (there is no CPU path)")
    if not (isinstance(kernel, torch.Tensor) and kernel.dtype == torch.float32):
        raise TypeError("kernel must be a float32 tensor on a GPU (there is no CPU path)")
    if images.dim() != 4 or images.shape[3] != 3 or kernel.dim() != 4 or tuple(kernel.shape[:3]) != (3, 3, 3):
        raise ValueError("images must be [B,H,W,3] and kernel [3,3,3,Cout]")
    if (images.shape[1] | images.shape[2]) & 1:
        raise ValueError("images: even height and width (the network's size)")
    if kernel.shape[3] % 4 or not 4 <= kernel.shape[3] <= 64:
        raise ValueError("kernel: Cout must be a multiple of 4 and at most 64")
    if not (images.is_cuda and kernel.is_cuda):
        raise TypeError("images and kernel must be on a GPU (there is no CPU path)")
    return _FirstConv.apply(images, kernel)


# ----------------------------------------------------------------------------- the batch norm
_ACTS = {"relu": 1, "relu6": 2}                                                # SSD_ACT_RELU, SSD_ACT_RELU6


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


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, epsilon, one_minus_momentum, act, *t):
        xs = tuple(x.contiguous() for x in t[:n])
        gammas, betas, mms, mvs = t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n], t[4 * n:5 * n]
        C, dev = xs[0].shape[-1], xs[0].device
        outs = tuple(torch.empty_like(x) for x in xs)
        Cp = (C + 3) // 4 * 4                                                  # rows of 16-byte multiples: every vector is aligned for any C
        stats = torch.empty((n, 3, Cp), dtype=torch.float32, device=dev)      # mean, var, invstd per level
        means, vars_, invstds = [stats[i, 0, :C] for i in range(n)], [stats[i, 1, :C] for i in range(n)], [stats[i, 2, :C] for i in range(n)]
        lv = _bn_levels(xs, None, outs, gammas, betas, mms, mvs, means, vars_, invstds, None, None)
        _bn_call(lib().ssd_bn_act_train_forward, lv, n, C, dev, act, 1, epsilon, one_minus_momentum)
        ctx.save_for_backward(stats, *(xs + tuple(gammas) + tuple(betas)))
        ctx.n, ctx.act = n, act
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
        _bn_call(lib().ssd_bn_act_train_backward, lv, n, C, dev, ctx.act)
        return (None, None, None, None) + dxs + tuple(dgammas) + tuple(dbetas) + (None,) * (2 * n)


def batch_norm_relu(x, gamma, beta, moving_mean, moving_variance, training, momentum=BATCH_NORM_MOMENTUM, epsilon=BATCH_NORM_EPSILON):
    """batch_norm_act with act="relu" (layer_utils.py:5-12)."""
    return batch_norm_act(x, gamma, beta, moving_mean, moving_variance, training, momentum, epsilon, act="relu")


def batch_norm_act(x, gamma, beta, moving_mean, moving_variance, training, momentum=BATCH_NORM_MOMENTUM, epsilon=BATCH_NORM_EPSILON,
                   act="relu6"):
    """Batch norm + ReLU (act="relu", layer_utils.py:5-12) or ReLU6 (act="relu6", mobilenet_v1.py:22-41) of x [..., C] with its own gamma, beta and moving statistics [C] -- or of a LIST of
    levels, each argument then a list (one launch sequence for all of them).  training=True: the batch's statistics (biased
    variance), the moving statistics are updated in place (moving -= (moving - batch) * (1 - momentum), unbiased variance);
    gradients flow to x, gamma and beta.  training=False: the inference form (x - moving_mean) * sf + beta that the engine
    folds into its convolutions, bit for bit; no gradient."""
    single = isinstance(x, torch.Tensor)
    cols = [[v] if single else list(v) for v in (x, gamma, beta, moving_mean, moving_variance)]
    n = len(cols[0])
    if act not in _ACTS:
        raise ValueError("act must be 'relu' or 'relu6'")
    if n < 1 or n > 8 or any(len(c) != n for c in cols):
        raise ValueError("batch_norm_act takes 1 .. 8 levels, every argument one entry per level")
    C = cols[0][0].shape[-1]
    for i in range(n):
        for c, name in zip(cols, ("x", "gamma", "beta", "moving_mean", "moving_variance")):
            _need(c[i], name)
            if c[i].shape[-1] != C or (name != "x" and c[i].dim() != 1) or not (name == "x" or c[i].is_contiguous()):
                raise ValueError("%s of level %d: contiguous, %d channels" % (name, i, C))
    eps = float(np.float32(epsilon))
    if training:
        omm = float(np.float32(1.0 - momentum))
        outs = _BnAct.apply(n, eps, omm, _ACTS[act], *(cols[0] + cols[1] + cols[2] + cols[3] + cols[4]))
    else:
        xs = [v.detach().contiguous() for v in cols[0]]
        outs = [torch.empty_like(v) for v in xs]
        lv = _bn_levels(xs, None, outs, cols[1], cols[2], cols[3], cols[4], None, None, None, None, None)
        _bn_call(lib().ssd_bn_act_train_forward, lv, n, C, xs[0].device, _ACTS[act], 0, eps, 0.0)
    return outs[0] if single else list(outs)


# ----------------------------------------------------------------------------- a block's variables
class ReferenceVariables(torch.nn.Module):
    """The variables of one block of the reference's graph as a torch.nn.Module: every entry of `shapes` {reference name: shape},
    in that order, from `weights` {name: float32 array in TF layout}; attribute names are the reference names with "/" -> "__".
    moving_mean / moving_variance become buffers, everything else a Parameter.  initial(name, shape, rng) -> array or None is
    asked for a variable that `weights` lacks or holds in another shape; None leaves the KeyError / ValueError standing.  rng is
    ONE numpy default_rng(seed) per module, touched only by what `initial` draws."""

    def __init__(self, shapes, weights, initial, device=None, seed=0):
        super().__init__()
        self._names, self._stat_names = [], []
        rng = np.random.default_rng(seed)
        for name, shape in shapes.items():
            a = weights.get(name)
            if a is None or tuple(np.shape(a)) != tuple(shape):
                drawn = initial(name, shape, rng)
                a = a if drawn is None else drawn
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

    def batch_norm_relu(self, xs, scopes, act="relu"):
        """batch_norm_act of the levels xs, level i with the variables of the batch-norm scope scopes[i], in the module's mode."""
        return batch_norm_act(xs, *[[self.variable("%s/%s" % (s, leaf)) for s in scopes]
                                    for leaf in ("gamma", "beta", "moving_mean", "moving_variance")], training=self.training, act=act)
