"""The TRAIN ShuffleNet's references (include/ssd_hip.h, "the TRAIN ShuffleNet"): the transpose of concat_shuffle_split, the max
pool's gradient with the header's tie rule, the batch norm's float32 sequence without an activation, the shapes at which a copy
goes round its grid more than once, and ShuffleNet-v2 in torch on the CPU in a chosen dtype with FORCED ReLU gates."""
import numpy as np

from helpers import backbone_train_ref as bref
from helpers import head_train_ref as href
from helpers.first_conv_train_ref import pixel_table, torch_first_conv

f32 = np.float32
EPS, MOMENTUM = href.EPS, href.MOMENTUM
rel = href.rel
STAGES = ((2, 4), (3, 8), (4, 4))
COPY_MAX_BLOCKS = 256 * 32          # csrc/train_shufflenet.hip SN_COPY_MAX_BLOCKS: the copies' grid-stride block cap (256 threads each)


# ----------------------------------------------------------------------------- shuffle
def shuffle_transpose(dxo, dyo):
    """The backward of concat_shuffle_split: dz = [dxo | dyo] -> (dx, dy) with dx[i] = dz[2i], dy[i] = dz[2i+1]; a copy."""
    dz = np.concatenate([dxo, dyo], axis=-1)
    return np.ascontiguousarray(dz[..., 0::2]), np.ascontiguousarray(dz[..., 1::2])


def copy_rows_past_one_grid_pass(D):
    """Rows of a [rows, D] copy whose thread count (rows * D / V, V the access width in words) exceeds what one pass of the capped
    grid covers, by a little and not by a multiple."""
    V = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    per_pass = COPY_MAX_BLOCKS * 256
    rows = -(-per_pass // (D // V)) + 37
    assert rows * (D // V) > per_pass and (rows * (D // V)) % per_pass
    return rows


# ----------------------------------------------------------------------------- max pool
def maxpool_forward(x):
    """3x3 stride 2 'SAME' on even sizes: m = a > m ? a : m from -inf over the taps row-major, cells beyond the edge outside."""
    B, H, W, C = x.shape
    out = np.full((B, H // 2, W // 2, C), -np.inf, f32)
    with np.errstate(invalid="ignore"):
        for ky in range(3):
            for kx in range(3):
                tap = x[:, ky::2, kx::2][:, :H // 2, :W // 2]
                o = out[:, :tap.shape[1], :tap.shape[2]]
                o[...] = np.where(tap > o, tap, o)
    return out


def maxpool_grad(x, dy):
    """The header's gradient: the winner of a window is the FIRST tap in row-major order whose value equals the window's output (a
    window whose output equals none of its taps has none); dx is the float32 sum of dy over the windows a position wins, one
    addition at a time from +0 in ascending (oy, ox)."""
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    B, H, W, C = x.shape
    out = maxpool_forward(x)
    dx = np.zeros_like(x)
    with np.errstate(invalid="ignore"):
        for oy in range(H // 2):
            for ox in range(W // 2):
                taken = np.zeros((B, C), bool)
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy + ky, 2 * ox + kx
                        if iy >= H or ix >= W:
                            continue
                        win = (x[:, iy, ix] == out[:, oy, ox]) & ~taken
                        taken |= win
                        dx[:, iy, ix] = np.where(win, (dx[:, iy, ix] + dy[:, oy, ox]).astype(f32), dx[:, iy, ix])
    return dx


def torch_maxpool(x, dy):
    """F.max_pool2d of the input padded with -inf at the bottom and right, float64 autograd -> (y, dx) numpy NHWC."""
    import torch
    import torch.nn.functional as F
    tx = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    y = F.max_pool2d(F.pad(tx.permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf")), 3, 2).permute(0, 2, 3, 1)
    y.backward(torch.tensor(np.asarray(dy, np.float64)))
    return y.detach().numpy(), tx.grad.numpy()


# ----------------------------------------------------------------------------- the batch norm without an activation
def bn_none_f32(x, gamma, beta, mean, invstd, dy=None, dgamma=None, dbeta=None):
    """The header's float32 operation sequence with SSD_ACT_NONE on given float32 statistics: out = y and, with dy, dgamma and
    dbeta, dx with g = dy."""
    x, gamma, beta, mean, invstd = (np.asarray(v, f32) for v in (x, gamma, beta, mean, invstd))
    with np.errstate(invalid="ignore", over="ignore"):
        t = x - mean
        sf = gamma * invstd
        y = (t * sf).astype(f32) + beta
        if dy is None:
            return y.astype(f32)
        R = f32(x.size // x.shape[-1])
        xh = t * invstd
        u = np.asarray(dy, f32) - (np.asarray(dbeta, f32) / R)
        v = xh * (np.asarray(dgamma, f32) / R)
        dx = sf * (u - v)
    return y.astype(f32), dx.astype(f32)


# ----------------------------------------------------------------------------- ShuffleNet-v2 in torch on the CPU
def relu_layers(features):
    """The layers of a run's features that end in a ReLU: every batch norm but the depthwise ones."""
    return [k for k in features if k == "Conv1" or k == "Conv5" or "conv1x1" in k]


def gates_of(features):
    """{layer: post-activation array} -> {layer: open} for the ReLU layers: v > 0."""
    return {k: features[k] > 0 for k in relu_layers(features)}


def torch_shufflenet(W, images, dtype, gates):
    """shufflenet_v2() (shufflenet_v2.py:7-137) from the uint8 frames in torch ops of `dtype` on the CPU, every batch norm on batch
    statistics.  The ReLU gates are FORCED: out = y * gates[layer], so that runs in different precisions differentiate the same
    piecewise-linear function; the max pool is torch's (a tie at zero sits behind a closed gate).  -> ([c3, c4, c5] NHWC tensors,
    T {name: leaf tensor of every trainable variable, TF layout}, S {name: updated moving statistic}, raw {1x1 layer: its raw output
    NCHW -- the input of its batch norm --, which keeps its gradient after a backward})."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in W.items()
         if k.startswith("ShuffleNetV2/") and k.rsplit("/", 1)[1] in ("weights", "depthwise_weights", "gamma", "beta")}
    omm = float(f32(1.0 - MOMENTUM)) if dtype == torch.float32 else 1.0 - MOMENTUM
    S, raw = {}, {}

    def bn(v, scope, relu):
        s = "ShuffleNetV2/" + scope + "/batch_norm"
        g, b = T[s + "/gamma"].view(1, -1, 1, 1), T[s + "/beta"].view(1, -1, 1, 1)
        mm = torch.tensor(np.asarray(W[s + "/moving_mean"], np.float64), dtype=dtype)
        mv = torch.tensor(np.asarray(W[s + "/moving_variance"], np.float64), dtype=dtype)
        mean = v.mean((0, 2, 3))
        var = ((v - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        rows = v.numel() // v.shape[1]
        S[s + "/moving_mean"] = mm - (mm - mean.detach()) * omm
        S[s + "/moving_variance"] = mv - (mv - var.detach() * (rows / (rows - 1.0))) * omm
        y = (v - mean.view(1, -1, 1, 1)) * (g / torch.sqrt(var.view(1, -1, 1, 1) + EPS)) + b
        if not relu:
            return y
        return y * torch.tensor(np.ascontiguousarray(gates[scope].transpose(0, 3, 1, 2)).astype(np.float64), dtype=dtype)

    def conv(x, scope):
        raw[scope] = F.conv2d(x, T["ShuffleNetV2/" + scope + "/weights"].permute(3, 2, 0, 1))
        raw[scope].retain_grad()
        return bn(raw[scope], scope, True)

    def dw(x, scope, stride):
        C, H, Wd = x.shape[1], x.shape[2], x.shape[3]
        (OH, pt), (OW, pl) = bref.same(H, stride), bref.same(Wd, stride)
        pb, pr = max((OH - 1) * stride + 3 - H, 0) - pt, max((OW - 1) * stride + 3 - Wd, 0) - pl
        k = T["ShuffleNetV2/" + scope + "/depthwise_weights"].permute(2, 3, 0, 1)
        return bn(F.conv2d(F.pad(x, (pl, pr, pt, pb)), k, stride=stride, groups=C), scope, False)

    x = torch.tensor(pixel_table()[images].astype(np.float64), dtype=dtype).permute(0, 3, 1, 2)         # exact in either dtype
    x = bn(torch_first_conv(x, T["ShuffleNetV2/Conv1/weights"]), "Conv1", True)
    x = F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=float("-inf")), 3, 2)
    outs = []
    for stage, units in STAGES:
        u = "Stage%d/unit_1" % stage
        y = conv(dw(conv(x, u + "/conv1x1_before"), u + "/depthwise", 2), u + "/conv1x1_after")
        x = conv(dw(x, u + "/second_branch/depthwise", 2), u + "/second_branch/conv1x1_after")
        for j in range(2, units + 1):
            D = x.shape[1]
            z = torch.stack([x, y], dim=2).reshape(x.shape[0], 2 * D, x.shape[2], x.shape[3])      # z[2i] = x[i], z[2i+1] = y[i]
            x, y = z[:, :D], z[:, D:]
            u = "Stage%d/unit_%d" % (stage, j)
            x = conv(dw(conv(x, u + "/conv1x1_before"), u + "/depthwise", 1), u + "/conv1x1_after")
        x = torch.cat([x, y], dim=1)
        outs.append(x)
    outs[2] = conv(x, "Conv5")
    return [o.permute(0, 2, 3, 1) for o in outs], T, S, raw


# ----------------------------------------------------------------------------- the 19 betas whose gradient is zero
def dead_betas(names):
    """The beta of every depthwise batch norm: a per-channel constant that a bias-free 1x1 convolution carries into a batch norm on
    batch statistics, which subtracts it again.  The loss does not depend on it: its gradient is zero in exact arithmetic, and what a
    float run holds there is rounding residue."""
    return [n for n in names if n.endswith("depthwise/batch_norm/beta")]


def dead_beta_bound(W, raw, name):
    """A bound on |d beta| of the depthwise batch norm `name` for any float32 evaluation, from a float64 run's `raw` (after its
    backward).  d beta[ci] = sum_r g[r,ci] with g = the data gradient of the 1x1 convolution that follows, g[r,ci] = sum_co
    d[r,co] * w[ci,co], d the gradient at that convolution's output.  sum_r d[r,co] = 0 exactly (it is the dx of a batch norm on batch
    statistics), so the exact sum is 0 and what remains is the rounding of the terms: a chain of K = Cout fmafs per g is off by at most
    K u sum_co |d * w| (u = 2^-24), and d itself comes from a handful of float32 operations of the batch norm's backward, for which
    16 u of the same scale is allowed.  -> [C] float64: (K + 16) * 2^-24 * sum_r sum_co |d[r,co]| * |w[ci,co]|."""
    scope = name[len("ShuffleNetV2/"):-len("/depthwise/batch_norm/beta")] + "/conv1x1_after"
    d = np.abs(raw[scope].grad.numpy().astype(np.float64)).sum((0, 2, 3))                # [Cout]
    w = np.abs(np.asarray(W["ShuffleNetV2/" + scope + "/weights"], np.float64))[0, 0]    # [Cin, Cout]
    return (w.shape[1] + 16) * 2.0 ** -24 * (w @ d)
