"""The differentiable ops under the trainable modules (include/ssd_hip.h, "the TRAIN head", "the TRAIN FPN" and "the TRAIN
backbone", "the TRAIN first convolution" (from uint8 and from float frames) and "the TRAIN ShuffleNet"), and nothing about any model: conv_same / conv3x3_same,
depthwise_conv, pointwise_conv, first_conv_train, first_conv_train_float, batch_norm_act (batch_norm_relu is its act="relu" case), concat_shuffle_split,
concat_channels and maxpool3x3s2_train are torch.autograd.Functions over the C entry points (once differentiable), fpn_merge_backward is
ssd_fpn_merge_backward, and ReferenceVariables is the torch.nn.Module base that holds a block's variables under their reference
names.  The Functions allocate the results and keep what the backward needs; how an entry point is called (the level structs, the
argument order, the workspace, the stream, the shape checks) is train_calls.py's, where fpn_merge_backward lives too.  torch
provides memory, streams and the autograd graph only.  head_train.py, fpn_train.py, backbone_train.py and shufflenet_train.py build
RetinaNetBoxPredictor, fpn(), mobilenet_v1() and shufflenet_v2() from these.
depthwise_conv, pointwise_conv and batch_norm_act go to the TRAIN ShuffleNet's entry points exactly where the older ones refuse -- a
channel count that is 2 mod 4, act="none" -- so every shape they took before keeps its launches and bits.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import train_calls as calls
from .train_calls import _need, fpn_merge_backward                             # noqa: F401  (re-exported)

BATCH_NORM_MOMENTUM = 0.993     # detector/constants.py
BATCH_NORM_EPSILON = 1e-3


# ----------------------------------------------------------------------------- the convolution
def _conv_forward(xs, kernel, bias, stride, ups, entry="conv"):
    """train_calls.conv_forward on contiguous levels -> the outputs."""
    outs = tuple(torch.empty(calls.conv_out_shape(x.shape, kernel.shape[3], stride), dtype=torch.float32, device=kernel.device) for x in xs)
    calls.conv_forward(xs, kernel, outs, stride, bias, ups, entry=entry)
    return outs


def _conv_backward(xs, kernel, dys, stride, want_dx, want_dbias=False, entry="conv"):
    """train_calls.conv_backward -> (dw, dbias or None, dxs or None); entry "pointwise": the k = 1 call that gives the data gradient."""
    dxs = tuple(torch.empty_like(x) for x in xs) if want_dx else None
    dw = torch.empty_like(kernel)
    dbias = torch.empty(kernel.shape[3], dtype=torch.float32, device=kernel.device) if want_dbias else None
    calls.conv_backward(xs, kernel, dys, dw, stride, dxs, dbias, entry=entry)
    return dw, dbias, dxs


class _Conv(torch.autograd.Function):
    """(kernel, bias, stride, pointwise, n, the n levels, then one `up` per level or none) -> the n outputs.  pointwise: the backward
    is ssd_pointwise_train_backward, which gives a 1x1 convolution's data gradient; pointwise == "sn_pointwise" (Cin = 2 mod 4): the
    TRAIN ShuffleNet's pair, forward and backward."""

    @staticmethod
    def forward(ctx, kernel, bias, stride, pointwise, n, *t):
        xs = tuple(x.contiguous() for x in t[:n])
        ups = tuple(u.contiguous() for u in t[n:]) if len(t) > n else None
        kernel = kernel.contiguous()
        outs = _conv_forward(xs, kernel, bias, stride, ups, "sn_pointwise" if pointwise == "sn_pointwise" else "conv")
        ctx.save_for_backward(kernel, *xs)
        ctx.stride, ctx.pointwise, ctx.n, ctx.has_bias, ctx.has_up = stride, pointwise, n, bias is not None, ups is not None
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        kernel, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        n, Cout = ctx.n, kernel.shape[3]
        dys = tuple(torch.zeros(calls.conv_out_shape(x.shape, Cout, ctx.stride), dtype=torch.float32, device=x.device) if d is None else d.contiguous()
                    for x, d in zip(xs, dys))
        want_dx = any(ctx.needs_input_grad[5:5 + n])
        if want_dx and kernel.shape[0] == 1 and not ctx.pointwise:
            raise RuntimeError("conv_same: a 1x1 convolution has no data gradient here (nothing trainable lies upstream of a lateral "
                               "while the backbone is frozen); detach its input")
        entry = ctx.pointwise if ctx.pointwise == "sn_pointwise" else "pointwise" if ctx.pointwise else "conv"
        dw, dbias, dxs = _conv_backward(xs, kernel, dys, ctx.stride, want_dx, ctx.has_bias, entry)
        dups = ()
        if ctx.has_up:                                                  # the gradient of `up`: the 2x2 sums of dy
            dups = tuple(fpn_merge_backward(d) if need else None for d, need in zip(dys, ctx.needs_input_grad[5 + n:]))
        return (dw, dbias, None, None, None) + (dxs if want_dx else (None,) * n) + dups


def _level_list(features, kernel, who, kernel_ok, kernel_shape):
    """What conv_same and pointwise_conv ask of their levels and their ONE kernel -> (features is a single tensor, the levels)."""
    single = isinstance(features, torch.Tensor)
    xs = [features] if single else list(features)
    if not xs or len(xs) > 8:
        raise ValueError("%s takes 1 .. 8 levels" % who)
    _need(kernel, "kernel")
    if kernel.dim() != 4 or not kernel_ok(tuple(kernel.shape)):
        raise ValueError("kernel must be HWIO %s" % kernel_shape)
    for x in xs:
        _need(x, "features")
        if x.dim() != 4 or x.shape[3] != kernel.shape[2] or x.shape[0] != xs[0].shape[0]:
            raise ValueError("every level must be [B,H,W,Cin] with the kernel's Cin and one batch size")
    return single, xs


def conv_same(features, kernel, stride=1, up=None, bias=None):
    """conv2d_same (layer_utils.py:15-43) of every level with ONE kernel: features a tensor [B,H,W,Cin] or a list of them, kernel
    HWIO [k,k,Cin,Cout] with k = 1 or 3, stride 1 or 2 (2 only with k = 3: the output is ceil(H/2) x ceil(W/2), an explicit pad of 1),
    up (stride 1, even H and W only) a tensor [B,H/2,W/2,Cout] per level that is added after nearest x2 upsampling.  All float32
    CUDA tensors; returns the same kind as `features`.  The forward is bit-identical to ssd_amd.ssd.conv2d with the same arguments
    (mode "EXPLICIT" for stride 2).  Gradients flow to the kernel, the bias, `up` (the 2x2 sums of the output's gradient) and, for
    k = 3, to the features; a 1x1 convolution whose input requires a gradient raises in backward."""
    single, xs = _level_list(features, kernel, "conv_same", lambda s: s[0] == s[1] and s[0] in (1, 3), "[k,k,Cin,Cout] with k = 1 or 3")
    if stride not in (1, 2) or (stride == 2 and kernel.shape[0] != 3):
        raise ValueError("stride must be 1 or 2, and 2 only with k = 3")
    if bias is not None:
        _need(bias, "bias")
        if tuple(bias.shape) != (kernel.shape[3],):
            raise ValueError("bias must have shape [Cout]")
    ups = []
    if up is not None:
        ups = [up] if isinstance(up, torch.Tensor) else list(up)
        if stride != 1 or bias is not None or len(ups) != len(xs):
            raise ValueError("up: one tensor per level, only with stride 1 and without a bias")
        for x, u in zip(xs, ups):
            _need(u, "up")
            if (x.shape[1] | x.shape[2]) & 1 or tuple(u.shape) != (x.shape[0], x.shape[1] // 2, x.shape[2] // 2, kernel.shape[3]):
                raise ValueError("up must be [B,H/2,W/2,Cout] of a level with even H and W")
    outs = _Conv.apply(kernel, bias, stride, False, len(xs), *(xs + ups))
    return outs[0] if single else list(outs)


def conv3x3_same(features, kernel, bias=None):
    """conv_same for the head: kernel HWIO [3,3,Cin,Cout], stride 1 (+ bias).  The forward is bit-identical to ssd_amd.ssd.conv2d;
    gradients flow to the features, the kernel and the bias."""
    _need(kernel, "kernel")
    if kernel.dim() != 4 or tuple(kernel.shape[:2]) != (3, 3):
        raise ValueError("kernel must be HWIO [3,3,Cin,Cout]")
    return conv_same(features, kernel, bias=bias)


# ----------------------------------------------------------------------------- the backbone's convolutions
def pointwise_conv(features, kernel):
    """slim.conv2d 1x1, stride 1, raw (mobilenet_v1.py:66 before its batch norm): features a tensor [B,H,W,Cin] or a list of them that
    share ONE kernel HWIO [1,1,Cin,Cout], Cin a multiple of 4 -- or 2 mod 4 with an even Cout (ShuffleNet's 58), which takes the TRAIN
    ShuffleNet's entry points.  The forward is conv_same's (bit-identical to ssd_amd.ssd.conv2d);
    gradients flow to the kernel AND to the features (dx = conv1x1(dy, kernel transposed), one fmaf chain per element)."""
    single, xs = _level_list(features, kernel, "pointwise_conv", lambda s: s[:2] == (1, 1), "[1,1,Cin,Cout]")
    outs = _Conv.apply(kernel, None, 1, "sn_pointwise" if kernel.shape[2] % 4 == 2 else True, len(xs), *xs)
    return outs[0] if single else list(outs)


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride):
        x, kernel = x.contiguous(), kernel.contiguous()
        out = torch.empty(calls.conv_out_shape(x.shape, x.shape[3], stride), dtype=torch.float32, device=x.device)
        ctx.entry = "sn_depthwise" if x.shape[3] % 4 == 2 else "depthwise"
        calls.depthwise_forward(x, kernel, out, stride, entry=ctx.entry)
        ctx.save_for_backward(x, kernel)
        ctx.stride = stride
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, kernel = ctx.saved_tensors
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(kernel)
        calls.depthwise_backward(x, kernel, dy.contiguous(), dw, ctx.stride, dx, entry=ctx.entry)
        return dx, dw, None


def depthwise_conv(x, kernel, stride=1):
    """tf.nn.depthwise_conv2d, 3x3, 'SAME', raw (depthwise_conv.py:5-26 before its batch norm): x [B,H,W,C], kernel [3,3,C,1], C a
    multiple of 4 -- or 2 mod 4, on the TRAIN ShuffleNet's entry points -- (at most 1024 for the backward), stride 1 or 2 (2: H and W of one parity).  The forward is bit-identical to
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
        out = torch.empty((B, H // 2, W // 2, kernel.shape[3]), dtype=torch.float32, device=images.device)
        calls.first_conv_forward(images, kernel, out)
        ctx.save_for_backward(images)
        ctx.Cout = kernel.shape[3]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        images, = ctx.saved_tensors
        dw = torch.empty((3, 3, 3, ctx.Cout), dtype=torch.float32, device=images.device)
        calls.first_conv_backward(images, dy.contiguous(), dw)
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


class _FirstConvFloat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, kernel):
        images, kernel = images.contiguous(), kernel.contiguous()
        B, H, W, _ = images.shape
        out = torch.empty((B, H // 2, W // 2, kernel.shape[3]), dtype=torch.float32, device=images.device)
        calls.first_conv_f32_forward(images, kernel, out)
        ctx.save_for_backward(images)
        ctx.Cout = kernel.shape[3]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        images, = ctx.saved_tensors
        dw = torch.empty((3, 3, 3, ctx.Cout), dtype=torch.float32, device=images.device)
        calls.first_conv_f32_backward(images, dy.contiguous(), dw)
        return None, dw


def first_conv_train_float(images, kernel):
    """first_conv_train on the batches TrainPipeline yields: images float32 [B,H,W,3] in [0, 1] on the GPU at the network's own size
    (H and W even), kernel [3,3,3,Cout], Cout a multiple of 4 and at most 64.  The pixel value is the reference's 2 * x - 1
    (mobilenet_v1.py:34), one rounding, no clamp: on frames u * (1 / 255) the forward and the kernel's gradient have the bits of
    first_conv_train on the bytes u.  The gradient flows to the kernel only (the input is the image; it must not require one)."""
    if not (isinstance(images, torch.Tensor) and images.dtype == torch.float32):
        raise TypeError("images must be a float32 tensor on a GPU (there is no CPU path)")
    if not (isinstance(kernel, torch.Tensor) and kernel.dtype == torch.float32):
        raise TypeError("kernel must be a float32 tensor on a GPU (there is no CPU path)")
    if images.dim() != 4 or images.shape[3] != 3 or kernel.dim() != 4 or tuple(kernel.shape[:3]) != (3, 3, 3):
        raise ValueError("images must be [B,H,W,3] and kernel [3,3,3,Cout]")
    if (images.shape[1] | images.shape[2]) & 1:
        raise ValueError("images: even height and width (the network's size)")
    if kernel.shape[3] % 4 or not 4 <= kernel.shape[3] <= 64:
        raise ValueError("kernel: Cout must be a multiple of 4 and at most 64")
    if images.requires_grad:
        raise ValueError("images must not require a gradient: the first convolution has no data gradient")
    if not (images.is_cuda and kernel.is_cuda):
        raise TypeError("images and kernel must be on a GPU (there is no CPU path)")
    return _FirstConvFloat.apply(images, kernel)


# ----------------------------------------------------------------------------- the batch norm
def _rows(buf, C):
    """buf [n, m, Cp] -> m lists of the n levels' [C] vectors: rows of 16-byte multiples, so every vector is aligned for any C."""
    return [[buf[i, j, :C] for i in range(buf.shape[0])] for j in range(buf.shape[1])]


def _bn_entry(act):
    """act "none" (ShuffleNet's depthwise layers) is the TRAIN ShuffleNet's pair; the others keep theirs."""
    return "sn_bn" if act == "none" else "bn_act"


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, epsilon, one_minus_momentum, act, *t):
        xs = tuple(x.contiguous() for x in t[:n])
        gammas, betas, mms, mvs = t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n], t[4 * n:5 * n]
        C = xs[0].shape[-1]
        outs = tuple(torch.empty_like(x) for x in xs)
        stats = torch.empty((n, 3, (C + 3) // 4 * 4), dtype=torch.float32, device=xs[0].device)      # mean, var, invstd per level
        calls.bn_forward(xs, outs, gammas, betas, True, epsilon, one_minus_momentum, mms, mvs, *_rows(stats, C), act=act, entry=_bn_entry(act))
        ctx.save_for_backward(stats, *(xs + tuple(gammas) + tuple(betas)))
        ctx.n, ctx.act = n, act
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        n = ctx.n
        stats, t = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        xs, gammas, betas = t[:n], t[n:2 * n], t[2 * n:3 * n]
        C = xs[0].shape[-1]
        dys = tuple(torch.zeros_like(x) if d is None else d.contiguous() for x, d in zip(xs, dys))
        dxs = tuple(torch.empty_like(x) for x in xs)
        grads = torch.empty((n, 2, (C + 3) // 4 * 4), dtype=torch.float32, device=xs[0].device)
        dgammas, dbetas = _rows(grads, C)
        means, _, invstds = _rows(stats, C)
        calls.bn_backward(xs, dys, dxs, gammas, betas, means, invstds, dgammas, dbetas, act=ctx.act, entry=_bn_entry(ctx.act))
        return (None, None, None, None) + dxs + tuple(dgammas) + tuple(dbetas) + (None,) * (2 * n)


def batch_norm_relu(x, gamma, beta, moving_mean, moving_variance, training, momentum=BATCH_NORM_MOMENTUM, epsilon=BATCH_NORM_EPSILON):
    """batch_norm_act with act="relu" (layer_utils.py:5-12)."""
    return batch_norm_act(x, gamma, beta, moving_mean, moving_variance, training, momentum, epsilon, act="relu")


def batch_norm_act(x, gamma, beta, moving_mean, moving_variance, training, momentum=BATCH_NORM_MOMENTUM, epsilon=BATCH_NORM_EPSILON,
                   act="relu6"):
    """Batch norm + ReLU (act="relu", layer_utils.py:5-12), ReLU6 (act="relu6", mobilenet_v1.py:22-41) or no activation (act="none",
    shufflenet_v2.py:121,131,135) of x [..., C] with its own gamma, beta and moving statistics [C] -- or of a LIST of
    levels, each argument then a list (one launch sequence for all of them).  training=True: the batch's statistics (biased
    variance), the moving statistics are updated in place (moving -= (moving - batch) * (1 - momentum), unbiased variance);
    gradients flow to x, gamma and beta.  training=False: the inference form (x - moving_mean) * sf + beta that the engine
    folds into its convolutions, bit for bit; no gradient."""
    single = isinstance(x, torch.Tensor)
    cols = [[v] if single else list(v) for v in (x, gamma, beta, moving_mean, moving_variance)]
    n = len(cols[0])
    if act not in calls.SN_ACTS:
        raise ValueError("act must be 'relu', 'relu6' or 'none'")
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
        outs = _BnAct.apply(n, eps, omm, act, *(cols[0] + cols[1] + cols[2] + cols[3] + cols[4]))
    else:
        xs = [v.detach().contiguous() for v in cols[0]]
        outs = [torch.empty_like(v) for v in xs]
        calls.bn_forward(xs, outs, cols[1], cols[2], False, eps, 0.0, cols[3], cols[4], act=act, entry=_bn_entry(act))
    return outs[0] if single else list(outs)


# ----------------------------------------------------------------------------- ShuffleNet's copies and its max pool
def _pair(x, y, who):
    _need(x, "x")
    _need(y, "y")
    if x.dim() < 1 or x.shape != y.shape:
        raise ValueError("%s: x and y must be [..., D] tensors of one shape" % who)


class _Shuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        xo, yo = torch.empty_like(x), torch.empty_like(y)
        calls.shuffle(x, y, xo, yo)
        return xo, yo

    @staticmethod
    @once_differentiable
    def backward(ctx, dxo, dyo):
        dxo, dyo = dxo.contiguous(), dyo.contiguous()
        dx, dy = torch.empty_like(dxo), torch.empty_like(dyo)
        calls.shuffle(dxo, dyo, dx, dy, transpose=True)
        return dx, dy


def concat_shuffle_split(x, y):
    """concat_shuffle_split (shufflenet_v2.py:94-115) of x, y [..., D]: z[2i] = x[i], z[2i+1] = y[i] -> (z[:D], z[D:]), a copy of bit
    patterns; the gradients of x and y are the transpose of that copy."""
    _pair(x, y, "concat_shuffle_split")
    return _Shuffle.apply(x, y)


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        out = torch.empty(x.shape[:-1] + (2 * x.shape[-1],), dtype=torch.float32, device=x.device)
        calls.concat(x, y, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        dx = torch.empty(g.shape[:-1] + (g.shape[-1] // 2,), dtype=torch.float32, device=g.device)
        dy = torch.empty_like(dx)
        calls.split(g, dx, dy)
        return dx, dy


def concat_channels(x, y):
    """tf.concat([x, y], axis=3) of two halves [..., D] (shufflenet_v2.py:89) -> [..., 2D]; the gradient splits again."""
    _pair(x, y, "concat_channels")
    return _Concat.apply(x, y)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from . import ssd
        x = x.contiguous()
        with torch.cuda.device(x.device):
            out = ssd.maxpool3x3s2(x)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        calls.maxpool_backward(x, dy.contiguous(), dx)
        return dx


def maxpool3x3s2_train(x):
    """slim.max_pool2d 3x3, stride 2, 'SAME' (shufflenet_v2.py:51-54) of x [B,H,W,C], H and W even, C a multiple of 4: the forward is
    ssd_amd.ssd.maxpool3x3s2; the gradient of a window goes to its first maximal tap in row-major order."""
    _need(x, "x")
    if x.dim() != 4 or (x.shape[1] | x.shape[2]) & 1 or x.shape[3] % 4:
        raise ValueError("x must be [B,H,W,C] with even H and W and C a multiple of 4")
    return _MaxPool.apply(x)


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
