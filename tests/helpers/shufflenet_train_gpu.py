"""GPU-side helpers shared by tests/test_gpu_shufflenet_train.py and tests/test_gpu_shufflenet_train_scale.py: the TRAIN
ShuffleNet's raw calls (include/ssd_hip.h, "the TRAIN ShuffleNet") through ssd.train_calls on numpy arrays, every output pre-filled
with NaN and every workspace of exactly the size its planner asks for."""
import numpy as np

from helpers import backbone_train_ref as bref
from helpers import head_train_ref as href
from helpers.head_train_gpu import dev, exact_workspace

f32 = np.float32


def dw_forward(ssd, cuda, x, k, stride, entry):
    """ssd_depthwise_train_forward / ssd_sn_depthwise_train_forward of x [B,H,W,C] with the kernel k [3,3,C,1] -> out as numpy."""
    X = dev(cuda, x)
    out = cuda.full((x.shape[0],) + bref.dw_out_hw(x.shape[1], x.shape[2], stride) + (x.shape[3],), float("nan"), device="cuda")
    ssd.train_calls.depthwise_forward(X, dev(cuda, k), out, stride, entry=entry)
    return out.cpu().numpy()


def pw(ssd, cuda, x, k, dy, entry):
    """The 1x1 forward and backward of one level (entry "sn_pointwise", or "pointwise": the forward is then ssd_conv_train_forward)
    -> (y, dx, dw) as numpy."""
    calls = ssd.train_calls
    X, K, DY = dev(cuda, x), dev(cuda, k), dev(cuda, dy)
    need = calls.conv_workspace_bytes([X], X.shape[0], k.shape[2], k.shape[3], 1, entry=entry)
    ws = exact_workspace(cuda, need)
    Y = cuda.full_like(DY, float("nan"))
    calls.conv_forward([X], K, [Y], workspace=None if entry == "pointwise" else ws, entry="conv" if entry == "pointwise" else entry)
    DX, DW = cuda.full_like(X, float("nan")), cuda.full_like(K, float("nan"))
    calls.conv_backward([X], K, [DY], DW, dxs=[DX], workspace=ws, entry=entry)
    return Y.cpu().numpy(), DX.cpu().numpy(), DW.cpu().numpy()


def bn_raw(ssd, cuda, x, gamma, beta, mm, mv, dy=None, training=1, act="none", entry="sn_bn"):
    """ssd_sn_bn_train_forward (and, with dy, _backward) of one level x [rows, C] -> a dict of numpy arrays: y, the moved mm and mv, dx
    with dy, and mean, var, invstd, dgamma, dbeta (rows of a table padded to a multiple of 4 channels: every pointer 16-byte aligned)."""
    calls = ssd.train_calls
    C = x.shape[-1]
    Cp = (C + 3) // 4 * 4
    X, G, Bt, MM, MV = (dev(cuda, v) for v in (x, gamma, beta, mm, mv))
    Y = cuda.full_like(X, float("nan"))
    st = cuda.full((5, Cp), float("nan"), device="cuda")
    mean, var, invstd, dgamma, dbeta = [[st[j, :C]] for j in range(5)]
    ws = exact_workspace(cuda, max(calls.bn_workspace_bytes([X], C), 256))
    calls.bn_forward([X], [Y], [G], [Bt], training, float(f32(href.EPS)), float(f32(1.0 - href.MOMENTUM)), [MM], [MV], mean, var, invstd,
                     act=act, workspace=ws, entry=entry)
    out = dict(y=Y, mm=MM, mv=MV)
    if dy is not None:
        DX = cuda.full_like(X, float("nan"))
        calls.bn_backward([X], [dev(cuda, dy)], [DX], [G], [Bt], mean, invstd, dgamma, dbeta, act=act, workspace=ws, entry=entry)
        out["dx"] = DX
    out.update(mean=st[0, :C], var=st[1, :C], invstd=st[2, :C], dgamma=st[3, :C], dbeta=st[4, :C])
    return {k: v.cpu().numpy() for k, v in out.items()}
