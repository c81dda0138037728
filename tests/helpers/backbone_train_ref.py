"""The TRAIN backbone's references (include/ssd_hip.h, "the TRAIN backbone"): the depthwise convolution's gradients restated (the
zero-dilated tensor E of the header's data gradient, the weight gradient's double products), torch autograd of the grouped
convolution with TF 'SAME' padding, the header's float32 sequence of the batch norm with ReLU or ReLU6, MobileNet-v1's Conv2d_1 ..
Conv2d_13 in torch on the CPU in a chosen dtype with FORCED ReLU6 gates, and fpn() with inputs that require a gradient."""
import numpy as np

from helpers import head_train_ref as href

f32 = np.float32
EPS, MOMENTUM = href.EPS, href.MOMENTUM
rel = href.rel
LAYERS = [(1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512), (1, 512), (1, 512), (1, 512), (1, 512), (1, 512), (2, 1024), (1, 1024)]


# ----------------------------------------------------------------------------- the depthwise convolution
def same(n, stride):
    """TF 'SAME' for a 3-wide window -> (output size, pad_beg)."""
    o = -(-n // stride)
    return o, max((o - 1) * stride + 3 - n, 0) // 2


def dw_out_hw(h, w, stride):
    return same(h, stride)[0], same(w, stride)[0]


def flip(w):
    """[3,3,C,1] rotated by 180 degrees."""
    return np.ascontiguousarray(w[::-1, ::-1])


def dilate_E(dy, H, W, stride):
    """The header's E [B,H,W,C]: zero except E[b, s*oy + 1 - p, s*ox + 1 - p, :] = dy[b,oy,ox,:] (stride 1: E = dy)."""
    (OH, p), (OW, pw) = same(H, stride), same(W, stride)
    assert p == pw and dy.shape[1:3] == (OH, OW)
    E = np.zeros((dy.shape[0], H, W, dy.shape[3]), dy.dtype)
    ys, xs = stride * np.arange(OH) + 1 - p, stride * np.arange(OW) + 1 - p
    assert ys.min() >= 0 and ys.max() < H and xs.min() >= 0 and xs.max() < W
    E[:, ys[:, None], xs[None, :]] = dy
    return E


def dw_terms(x, dy, stride):
    """The weight gradient's products: [rows, 9, C] float64, terms[r, ky*3+kx, c] = x[b,oy*s+ky-p,ox*s+kx-p,c] * dy[b,oy,ox,c] over the
    output rows r = (b*OH + oy)*OW + ox, zero where the position lies outside the input.  The product of two floats is exact."""
    B, H, W, C = x.shape
    (OH, p), (OW, _) = same(H, stride), same(W, stride)
    xp = np.zeros((B, H + 4, W + 4, C), np.float64)
    xp[:, 2:2 + H, 2:2 + W] = x
    t = np.zeros((B, OH, OW, 9, C), np.float64)
    d = dy.astype(np.float64)
    for ky in range(3):
        for kx in range(3):
            ys = stride * np.arange(OH) + ky - p + 2
            xs = stride * np.arange(OW) + kx - p + 2
            t[:, :, :, ky * 3 + kx] = xp[:, ys[:, None], xs[None, :]] * d
    return t.reshape(B * OH * OW, 9, C)


def torch_depthwise(x, w, stride, dy):
    """tf.nn.depthwise_conv2d 'SAME' as the grouped F.conv2d in float64 torch with autograd -> (y, dx, dw) numpy, NHWC / [3,3,C,1]."""
    import torch
    import torch.nn.functional as F
    B, H, W, C = x.shape
    (OH, pt), (OW, pl) = same(H, stride), same(W, stride)
    pb, pr = max((OH - 1) * stride + 3 - H, 0) - pt, max((OW - 1) * stride + 3 - W, 0) - pl
    tx = torch.tensor(x.astype(np.float64), requires_grad=True)
    tw = torch.tensor(w.astype(np.float64), requires_grad=True)
    y = F.conv2d(F.pad(tx.permute(0, 3, 1, 2), (pl, pr, pt, pb)), tw.permute(2, 3, 0, 1), stride=stride, groups=C).permute(0, 2, 3, 1)
    assert tuple(y.shape) == (B, OH, OW, C)
    y.backward(torch.tensor(dy.astype(np.float64)))
    return y.detach().numpy(), tx.grad.numpy(), tw.grad.numpy()


def slab_plan(rows, C):
    """The header's slab rule of the depthwise weight gradient (the batch norm's, one level) -> (rpp, slab_rows, slabs)."""
    return href.slab_plan([rows], C)


# ----------------------------------------------------------------------------- the batch norm with ReLU / ReLU6
def act_f32(y, act):
    """v = y > 0 ? y : 0; relu6: v = v < 6 ? v : 6 (a NaN gives 0)."""
    with np.errstate(invalid="ignore"):
        v = np.where(y > 0, y, f32(0))
        if act == "relu6":
            v = np.where(v < 6, v, f32(6))
    return v.astype(f32)


def gate_f32(y, act):
    with np.errstate(invalid="ignore"):
        return (y > 0) & (y < 6) if act == "relu6" else (y > 0)


def bn_act_f32(x, gamma, beta, mean, var, act, dy=None, dgamma=None, dbeta=None, eps=EPS, invstd=None):
    """The header's float32 operation sequence on given float32 statistics: (ypre, out) and, with dy, dgamma and dbeta, also dx."""
    x, gamma, beta, mean = (np.asarray(v, f32) for v in (x, gamma, beta, mean))
    invstd = href.invstd_f32(np.asarray(var, f32), eps) if invstd is None else np.asarray(invstd, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x - mean
        sf = gamma * invstd
        ypre = (t * sf).astype(f32) + beta
        out = act_f32(ypre, act)
        if dy is None:
            return ypre, out
        R = f32(x.size // x.shape[-1])
        xh = t * invstd
        g = np.where(gate_f32(ypre, act), np.asarray(dy, f32), f32(0))
        u = g - (np.asarray(dbeta, f32) / R)
        v = xh * (np.asarray(dgamma, f32) / R)
        dx = sf * (u - v)
    return ypre, out, dx.astype(f32)


# ----------------------------------------------------------------------------- Conv2d_1 .. 13 in torch on the CPU
def gates_of(features):
    """{layer name: post-activation array} of a run -> {layer name: (open, hi)}: 0 < v < 6 and v >= 6."""
    return {k: ((v > 0) & (v < 6), v >= 6) for k, v in features.items()}


def torch_mobilenet(W, x0, dtype, gates):
    """Conv2d_1 .. Conv2d_13 (mobilenet_v1.py:52-67) in torch ops of `dtype` on the CPU on batch statistics, x0 = Conv2d_0's output
    NHWC.  The ReLU6 gates are FORCED: layer by layer out = y * open + 6 * hi with (open, hi) = gates[layer name], so that runs in
    different precisions differentiate the same piecewise-linear function.  -> ([c3, c4, c5] NHWC tensors, T {name: leaf tensor of
    every trainable variable, TF layout}, S {name: updated moving statistic})."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in W.items()
         if k.startswith("MobilenetV1/") and not k.startswith("MobilenetV1/Conv2d_0/")
         and k.rsplit("/", 1)[1] in ("weights", "depthwise_weights", "gamma", "beta")}
    omm = float(f32(1.0 - MOMENTUM)) if dtype == torch.float32 else 1.0 - MOMENTUM
    S, outs = {}, []
    x = torch.tensor(x0.astype(np.float64), dtype=dtype).permute(0, 3, 1, 2)

    def bn_act(v, scope, layer):
        s = scope + "/BatchNorm"
        g, b = T[s + "/gamma"].view(1, -1, 1, 1), T[s + "/beta"].view(1, -1, 1, 1)
        mm = torch.tensor(np.asarray(W[s + "/moving_mean"], np.float64), dtype=dtype)
        mv = torch.tensor(np.asarray(W[s + "/moving_variance"], np.float64), dtype=dtype)
        mean = v.mean((0, 2, 3))
        var = ((v - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        rows = v.numel() // v.shape[1]
        S[s + "/moving_mean"] = mm - (mm - mean.detach()) * omm
        S[s + "/moving_variance"] = mv - (mv - var.detach() * (rows / (rows - 1.0))) * omm
        y = (v - mean.view(1, -1, 1, 1)) * (g / torch.sqrt(var.view(1, -1, 1, 1) + EPS)) + b
        opened, hi = gates[layer]
        opened = torch.tensor(np.ascontiguousarray(opened.transpose(0, 3, 1, 2)).astype(np.float64), dtype=dtype)
        hi = torch.tensor(np.ascontiguousarray(hi.transpose(0, 3, 1, 2)).astype(np.float64), dtype=dtype)
        return y * opened + 6.0 * hi

    for i, (stride, _f) in enumerate(LAYERS, 1):
        s = "MobilenetV1/Conv2d_%d_depthwise" % i
        C, H, Wd = x.shape[1], x.shape[2], x.shape[3]
        (OH, pt), (OW, pl) = same(H, stride), same(Wd, stride)
        pb, pr = max((OH - 1) * stride + 3 - H, 0) - pt, max((OW - 1) * stride + 3 - Wd, 0) - pl
        x = F.conv2d(F.pad(x, (pl, pr, pt, pb)), T[s + "/depthwise_weights"].permute(2, 3, 0, 1), stride=stride, groups=C)
        x = bn_act(x, s, "Conv2d_%d_depthwise" % i)
        s = "MobilenetV1/Conv2d_%d_pointwise" % i
        x = F.conv2d(x, T[s + "/weights"].permute(3, 2, 0, 1))
        x = bn_act(x, s, "Conv2d_%d_pointwise" % i)
        if i in (5, 11, 13):
            outs.append(x.permute(0, 2, 3, 1))
    return outs, T, S


# ----------------------------------------------------------------------------- fpn() with inputs that require a gradient
def torch_fpn_inputs(W, feats, dtype):
    """helpers.fpn_train_ref.torch_fpn's graph (feature_extractor.py:40-76, batch statistics) with c3, c4, c5 as leaves that require
    a gradient.  -> ([p3 .. p7] NHWC tensors, [c3, c4, c5] NHWC leaf tensors)."""
    import torch
    import torch.nn.functional as F
    K = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype) for k, v in W.items() if k.startswith("fpn/")}
    leaves = [torch.tensor(f.astype(np.float64), dtype=dtype, requires_grad=True) for f in feats]
    c = {i: t.permute(0, 3, 1, 2) for i, t in zip((3, 4, 5), leaves)}

    def conv2d_same(x, name, stride=1):
        w = K["fpn/%s/kernel" % name].permute(3, 2, 0, 1)
        k = w.shape[2]
        if stride == 1:
            return F.conv2d(x, w, padding=(k - 1) // 2)
        return F.conv2d(F.pad(x, (1, 1, 1, 1)), w, stride=stride)
    up = lambda x: x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    x = conv2d_same(c[5], "lateral5")
    raw = {5: conv2d_same(x, "p5"), 6: conv2d_same(c[5], "p6", 2)}
    raw[7] = conv2d_same(torch.relu(raw[6]), "p7", 2)
    for i in (4, 3):
        x = up(x) + conv2d_same(c[i], "lateral%d" % i)
        raw[i] = conv2d_same(x, "p%d" % i)
    outs = []
    for i in range(3, 8):
        s = "fpn/p%d_batch_norm" % i
        v = raw[i]
        mean = v.mean((0, 2, 3))
        var = ((v - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        y = (v - mean.view(1, -1, 1, 1)) * (K[s + "/gamma"].view(1, -1, 1, 1) / torch.sqrt(var.view(1, -1, 1, 1) + EPS)) + K[s + "/beta"].view(1, -1, 1, 1)
        outs.append(torch.relu(y).permute(0, 2, 3, 1))
    return outs, leaves
