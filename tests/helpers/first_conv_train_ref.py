"""The TRAIN first convolution's references (include/ssd_hip.h, "the TRAIN first convolution"): the 256 pixel values of the
inference path, the weight gradient's double products, torch autograd of the stride-2 convolution on the frame padded at the bottom
and right, and MobileNet-v1 from the uint8 frames -- Conv2d_0 on batch statistics in front of backbone_train_ref.torch_mobilenet's
graph -- in torch on the CPU in a chosen dtype with FORCED ReLU6 gates."""
import numpy as np

from helpers import backbone_train_ref as bref
from helpers.backbone_train_ref import slab_plan                      # noqa: F401  (the rule is the depthwise weight gradient's)
from helpers.head_train_ref import double_sum_bound, rel               # noqa: F401

f32 = np.float32
EPS, MOMENTUM = bref.EPS, bref.MOMENTUM
FIRST = "MobilenetV1/Conv2d_0"


def pixel_table():
    """p(u) = fp32(2 * fp32(u * inv255) - 1), inv255 = (float)(1.0 / 255.0), for u = 0 .. 255: float32 [256]."""
    inv255 = f32(1.0 / 255.0)
    v = (np.arange(256, dtype=f32) * inv255).astype(f32)
    return (f32(2.0) * v - f32(1.0)).astype(f32)


def fc_terms(images, dy):
    """The weight gradient's products: [R, 27, Cout] float64, terms[r, (ky*3+kx)*3+ci, co] = p(images[b,2oy+ky,2ox+kx,ci]) * dy[b,oy,ox,co]
    over the output rows r = (b*OH + oy)*OW + ox, zero where the position lies outside the input (row H, column W).  The product of
    two floats is exact in double."""
    B, H, W, _ = images.shape
    OH, OW = H // 2, W // 2
    assert dy.shape[:3] == (B, OH, OW)
    Cout = dy.shape[3]
    x = np.zeros((B, H + 2, W + 2, 3), np.float64)
    x[:, :H, :W] = pixel_table()[images].astype(np.float64)
    d = dy.astype(np.float64)
    t = np.zeros((B, OH, OW, 27, Cout), np.float64)
    for ky in range(3):
        for kx in range(3):
            tap = x[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]                 # [B,OH,OW,3]
            t[:, :, :, (ky * 3 + kx) * 3:(ky * 3 + kx) * 3 + 3] = tap[..., :, None] * d[..., None, :]
    return t.reshape(B * OH * OW, 27, Cout)


def torch_first_conv(x_nchw, w_hwio):
    """slim.conv2d 3x3 stride 2 'SAME' on even sizes: one row and one column of zeros at the bottom and right, then 'valid'."""
    import torch.nn.functional as F
    return F.conv2d(F.pad(x_nchw, (0, 1, 0, 1)), w_hwio.permute(3, 2, 0, 1), stride=2)


def torch_dw(images, dy):
    """dw [3,3,3,Cout] float64 by torch autograd of the float64 convolution."""
    import torch
    x = torch.tensor(pixel_table()[images].astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.zeros((3, 3, 3, dy.shape[3]), dtype=torch.float64, requires_grad=True)
    y = torch_first_conv(x, w).permute(0, 2, 3, 1)
    assert tuple(y.shape) == dy.shape
    y.backward(torch.tensor(dy.astype(np.float64)))
    return w.grad.numpy()


def torch_mobilenet_from_images(W, images, dtype, gates):
    """backbone_train_ref.torch_mobilenet with Conv2d_0 in front, on batch statistics, its kernel, gamma and beta leaves as well:
    images uint8 [B,H,W,3] -> ([c3, c4, c5] NHWC tensors, T {name: leaf of every trainable variable, 81}, S {name: updated moving
    statistic, 54}).  gates[layer] = (open, hi), "Conv2d_0" included."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in W.items()
         if k.startswith("MobilenetV1/") and k.rsplit("/", 1)[1] in ("weights", "depthwise_weights", "gamma", "beta")}
    omm = float(f32(1.0 - MOMENTUM)) if dtype == torch.float32 else 1.0 - MOMENTUM
    S, outs = {}, []

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

    x = torch.tensor(pixel_table()[images].astype(np.float64), dtype=dtype).permute(0, 3, 1, 2)     # exact in either dtype
    x = bn_act(torch_first_conv(x, T[FIRST + "/weights"]), FIRST, "Conv2d_0")
    for i, (stride, _f) in enumerate(bref.LAYERS, 1):
        s = "MobilenetV1/Conv2d_%d_depthwise" % i
        C, H, Wd = x.shape[1], x.shape[2], x.shape[3]
        (OH, pt), (OW, pl) = bref.same(H, stride), bref.same(Wd, stride)
        pb, pr = max((OH - 1) * stride + 3 - H, 0) - pt, max((OW - 1) * stride + 3 - Wd, 0) - pl
        x = F.conv2d(F.pad(x, (pl, pr, pt, pb)), T[s + "/depthwise_weights"].permute(2, 3, 0, 1), stride=stride, groups=C)
        x = bn_act(x, s, "Conv2d_%d_depthwise" % i)
        s = "MobilenetV1/Conv2d_%d_pointwise" % i
        x = F.conv2d(x, T[s + "/weights"].permute(3, 2, 0, 1))
        x = bn_act(x, s, "Conv2d_%d_pointwise" % i)
        if i in (5, 11, 13):
            outs.append(x.permute(0, 2, 3, 1))
    return outs, T, S
