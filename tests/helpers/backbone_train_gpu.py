"""GPU-side helpers shared by tests/test_gpu_backbone_train.py and tests/test_gpu_train_scale.py: the depthwise and the first
convolution's backward straight through the C ABI (include/ssd_hip.h, "the TRAIN backbone", "the TRAIN first convolution") on
device tensors, and bit equality on the device."""
from helpers.head_train_gpu import dev, stream


def dw_backward_dev(ssd, cuda, X, Wt, DY, stride, with_dx=True):
    """ssd_depthwise_train_backward on device tensors with a workspace of exactly the size its planner asks for; the outputs are
    pre-filled with NaN.  -> (dx or None, dw) on the device."""
    L = ssd.lib()
    DX = cuda.full_like(X, float("nan")) if with_dx else None
    DW = cuda.full_like(Wt, float("nan"))
    b, h, ww, C = X.shape
    need = L.ssd_depthwise_train_workspace_bytes(b, h, ww, C, stride)
    assert need > 0
    ws = cuda.empty(need, dtype=cuda.uint8, device="cuda")
    ssd._lib.check(L.ssd_depthwise_train_backward(X.data_ptr(), DY.data_ptr(), b, h, ww, C, Wt.data_ptr(), stride,
                                                  DX.data_ptr() if with_dx else None, DW.data_ptr(), ws.data_ptr(), ws.numel(), stream(cuda)))
    return DX, DW


def dw_backward_raw(ssd, cuda, x, w, dy, stride, with_dx=True):
    """dw_backward_dev on numpy arrays.  -> (dx or None, dw) as numpy."""
    DX, DW = dw_backward_dev(ssd, cuda, dev(cuda, x), dev(cuda, w), dev(cuda, dy), stride, with_dx)
    return DX.cpu().numpy() if with_dx else None, DW.cpu().numpy()


def fc_backward_dev(ssd, cuda, IMG, DY):
    """ssd_first_conv_train_backward on device tensors (IMG uint8 [B,H,W,3], DY [B,H/2,W/2,Cout]) with a workspace of exactly the
    planner's size; dw is pre-filled with NaN.  -> dw on the device."""
    L = ssd.lib()
    B, H, W, _ = IMG.shape
    Cout = DY.shape[3]
    DW = cuda.full((3, 3, 3, Cout), float("nan"), device="cuda")
    need = L.ssd_first_conv_train_workspace_bytes(B, H, W, Cout)
    assert need > 0
    ws = cuda.empty(need, dtype=cuda.uint8, device="cuda")
    ssd._lib.check(L.ssd_first_conv_train_backward(IMG.data_ptr(), DY.data_ptr(), B, H, W, Cout, DW.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   stream(cuda)))
    return DW


def same_bits_dev(cuda, a, b):
    """Bit equality of two float32 device tensors (0.0 and -0.0 differ; a NaN equals only the same NaN)."""
    return a.shape == b.shape and cuda.equal(a.contiguous().view(cuda.int32), b.contiguous().view(cuda.int32))


def frames_same_bits(cuda, big, small, ids_dev, chunk=1024):
    """big[b] has the bits of small[ids[b]] for every frame b, compared on the device in chunks of frames.  -> the first chunk's
    start that differs, or None."""
    for b0 in range(0, big.shape[0], chunk):
        if not same_bits_dev(cuda, big[b0:b0 + chunk], small[ids_dev[b0:b0 + chunk]]):
            return b0
    return None
