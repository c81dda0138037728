"""The references of the TRAIN first convolution from float frames (include/ssd_hip.h, the header block of that name): the pixel
value q(x) = fp32(2 * x - 1) in numpy float32, the weight gradient's double products on q -- first_conv_train_ref.fc_terms with q(x)
in place of the byte table --, torch autograd of the float64 convolution, the frames the tests use and the raw calls on device
tensors."""
import numpy as np

from helpers.first_conv_train_ref import torch_first_conv
from helpers.head_train_gpu import exact_workspace

f32 = np.float32
INV255 = f32(1.0 / 255.0)


def q(x):
    """q(x) = fp32(2 * x - 1) elementwise on a float32 array: 2 * x is exact, the subtraction rounds once."""
    x = np.asarray(x)
    assert x.dtype == f32
    return (f32(2.0) * x - f32(1.0)).astype(f32)


def byte_frames(u):
    """x = fp32(u * inv255) for bytes u: what ssd_augment computes first (augment.hip) -- float frames on the byte grid."""
    return (np.asarray(u, np.uint8).astype(f32) * INV255).astype(f32)


def fc_terms(images, dy):
    """[R, 27, Cout] float64, terms[r, (ky*3+kx)*3+ci, co] = q(images[b,2oy+ky,2ox+kx,ci]) * dy[b,oy,ox,co] over the output rows
    r = (b*OH + oy)*OW + ox, zero where the position lies outside the input (row H, column W).  The product of two floats is exact
    in double."""
    B, H, W, _ = images.shape
    OH, OW = H // 2, W // 2
    assert dy.shape[:3] == (B, OH, OW) and images.dtype == f32
    Cout = dy.shape[3]
    x = np.zeros((B, H + 2, W + 2, 3), np.float64)
    x[:, :H, :W] = q(images).astype(np.float64)
    d = dy.astype(np.float64)
    t = np.zeros((B, OH, OW, 27, Cout), np.float64)
    for ky in range(3):
        for kx in range(3):
            tap = x[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]                 # [B,OH,OW,3]
            t[:, :, :, (ky * 3 + kx) * 3:(ky * 3 + kx) * 3 + 3] = tap[..., :, None] * d[..., None, :]
    return t.reshape(B * OH * OW, 27, Cout)


def torch_dw(images, dy):
    """dw [3,3,3,Cout] float64 by torch autograd of the float64 convolution of q(images)."""
    import torch
    x = torch.tensor(q(images).astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.zeros((3, 3, 3, dy.shape[3]), dtype=torch.float64, requires_grad=True)
    y = torch_first_conv(x, w).permute(0, 2, 3, 1)
    assert tuple(y.shape) == dy.shape
    y.backward(torch.tensor(dy.astype(np.float64)))
    return w.grad.numpy()


def grid_frames(rng, B, H, W):
    """Frames on the 2^-12 grid in [0, 1] with 0, 1, 1/2 and 2^-12 planted on the last row and the last column."""
    img = (rng.integers(0, 4097, (B, H, W, 3)).astype(f32) * f32(2.0 ** -12)).astype(f32)
    plant = np.array([0.0, 1.0, 0.5, 2.0 ** -12], f32)
    img[:, H - 1, :, :] = plant[rng.integers(0, 4, (B, W, 3))]
    img[:, :, W - 1, :] = plant[rng.integers(0, 4, (B, H, 3))]
    return img


def full_mantissa_frames(rng, B, H, W):
    """Full-mantissa random float32 in [0, 1] -- a random 24-bit significand at a random exponent down to 2^-12, so the low bits
    are set at every magnitude, not the multiples of 2^-24 a uniform draw gives -- with exact 0, exact 1, 2^-24, 1 - 2^-24 and a
    subnormal planted on the last row and the last column."""
    m = (rng.integers(1 << 23, 1 << 24, (B, H, W, 3)).astype(np.float64) * 2.0 ** -24)          # [1/2, 1)
    img = (m * 2.0 ** -rng.integers(0, 12, (B, H, W, 3)).astype(np.float64)).astype(f32)
    assert img.min() > 0 and img.max() < 1
    plant = np.array([0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-40], f32)
    assert plant[3] < 1 and 0 < plant[4] < np.finfo(f32).tiny
    img[:, H - 1, :, :] = plant[rng.integers(0, 5, (B, W, 3))]
    img[:, :, W - 1, :] = plant[rng.integers(0, 5, (B, H, 3))]
    return img


def f32_backward_dev(ssd, cuda, IMG, DY, fill_ws=None):
    """ssd_first_conv_f32_train_backward on device tensors (IMG float32 [B,H,W,3], DY [B,H/2,W/2,Cout]) with a workspace of exactly
    the planner's size, pre-filled with `fill_ws` (a byte) when given; dw is pre-filled with NaN.  -> dw on the device."""
    DW = cuda.full((3, 3, 3, DY.shape[3]), float("nan"), device="cuda")
    ws = exact_workspace(cuda, ssd.train_calls.first_conv_f32_workspace_bytes(IMG, DY.shape[3]), fill_ws)
    ssd.train_calls.first_conv_f32_backward(IMG, DY, DW, workspace=ws)
    return DW


def f32_forward_dev(ssd, cuda, IMG, K):
    """ssd_first_conv_f32_train_forward on device tensors into an output pre-filled with NaN.  -> out on the device."""
    B, H, W, _ = IMG.shape
    OUT = cuda.full((B, H // 2, W // 2, K.shape[3]), float("nan"), device="cuda")
    ssd.train_calls.first_conv_f32_forward(IMG, K, OUT)
    return OUT
