"""GPU-side helpers shared by tests/test_gpu_backbone_train.py, tests/test_gpu_train_scale.py and tests/
test_gpu_shufflenet_train_scale.py: the depthwise and the first convolution's backward (include/ssd_hip.h, "the TRAIN backbone",
"the TRAIN first convolution"; entry "sn_depthwise": "the TRAIN ShuffleNet") through ssd.train_calls on device tensors, and bit
equality on the device."""
from helpers.head_train_gpu import dev, exact_workspace


def dw_backward_dev(ssd, cuda, X, Wt, DY, stride, with_dx=True, entry="depthwise"):
    """ssd_depthwise_train_backward (entry "sn_depthwise": ssd_sn_depthwise_train_backward) on device tensors with a workspace of
    exactly the size its planner asks for; the outputs are pre-filled with NaN.  -> (dx or None, dw) on the device."""
    DX = cuda.full_like(X, float("nan")) if with_dx else None
    DW = cuda.full_like(Wt, float("nan"))
    ws = exact_workspace(cuda, ssd.train_calls.depthwise_workspace_bytes(X, stride, entry=entry))
    ssd.train_calls.depthwise_backward(X, Wt, DY, DW, stride, DX, workspace=ws, entry=entry)
    return DX, DW


def dw_backward_raw(ssd, cuda, x, w, dy, stride, with_dx=True, entry="depthwise"):
    """dw_backward_dev on numpy arrays.  -> (dx or None, dw) as numpy."""
    DX, DW = dw_backward_dev(ssd, cuda, dev(cuda, x), dev(cuda, w), dev(cuda, dy), stride, with_dx, entry)
    return DX.cpu().numpy() if with_dx else None, DW.cpu().numpy()


def fc_backward_dev(ssd, cuda, IMG, DY, fill_ws=None):
    """ssd_first_conv_train_backward on device tensors (IMG uint8 [B,H,W,3], DY [B,H/2,W/2,Cout]) with a workspace of exactly the
    planner's size, pre-filled with `fill_ws` (a byte) when given; dw is pre-filled with NaN.  -> dw on the device."""
    DW = cuda.full((3, 3, 3, DY.shape[3]), float("nan"), device="cuda")
    ws = exact_workspace(cuda, ssd.train_calls.first_conv_workspace_bytes(IMG, DY.shape[3]), fill_ws)
    ssd.train_calls.first_conv_backward(IMG, DY, DW, workspace=ws)
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
