"""The TRAIN first convolution from float frames on the CPU (include/ssd_hip.h, the header block of that name): the premises of the
GPU tests -- q on the byte grid is the uint8 block's pixel table, the weight gradient's restatement against torch autograd, exactly
--, every refusal of the three entry points through the loaded library (they come before any HIP call, so no GPU is needed), the
checks of ssd_amd.train_calls on CPU tensors and the refusals of first_conv_train_float."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import first_conv_f32_ref as ref
from helpers import first_conv_train_ref as uref

f32 = np.float32
f64 = np.float64


def test_q_on_the_byte_grid_is_the_uint8_pixel_table_for_all_256_bytes():
    """q(fp32(u * inv255)) == p(u) bit for bit: the premise of every equivalence test between the float and the uint8 calls."""
    x = ref.byte_frames(np.arange(256, dtype=np.uint8))
    assert x.dtype == f32 and x[0] == 0 and x[255] == 1 and np.all(np.diff(x) > 0)
    got, want = ref.q(x), uref.pixel_table()
    assert got.dtype == f32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_q_is_one_rounding_without_clamp_or_special_case():
    """2 * x is exact in float32 (short of overflow), so q(x) is the float32 nearest to the real 2x - 1; values outside [0, 1], a
    subnormal, infinities and NaN go through as IEEE arithmetic takes them."""
    rng = np.random.default_rng(1)
    x = ref.full_mantissa_frames(rng, 2, 6, 8).reshape(-1)
    exact = 2.0 * x.astype(f64) - 1.0                                     # exact in double: 25 significant bits at most
    assert np.array_equal(ref.q(x), exact.astype(f32))
    odd = np.array([-0.25, 1.5, 1e-40, np.inf, -np.inf, 3e38], f32)
    with np.errstate(over="ignore", invalid="ignore"):
        got = ref.q(np.append(odd, f32(np.nan)))
    assert np.array_equal(got[:6], np.array([-1.5, 2.0, -1.0, np.inf, -np.inf, np.inf], f32)) and np.isnan(got[6])


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (6, 4)])
def test_the_weight_gradients_restatement_is_torch_autograd_exactly(H, W):
    """sum over the rows of fc_terms == the gradient of the float64 stride-2 convolution of q(frame) padded by one row and column at
    the bottom and right.  Frames on the 2^-12 grid: q is a multiple of 2^-11 of magnitude at most 1; integer dy in [-8, 8]: every
    term is a multiple of 2^-11 below 2^3, so both sums are exact."""
    rng = np.random.default_rng(H * 10 + W)
    B, Cout = 2, 8
    images = ref.grid_frames(rng, B, H, W)
    dy = rng.integers(-8, 9, (B, H // 2, W // 2, Cout)).astype(f32)
    terms = ref.fc_terms(images, dy)
    assert terms.shape == (B * (H // 2) * (W // 2), 27, Cout)
    units = terms * 2.0 ** 11
    assert np.array_equal(units, np.round(units)) and np.abs(units).sum(0).max() < 2.0 ** 53
    got = terms.sum(0).reshape(3, 3, 3, Cout)
    want = ref.torch_dw(images, dy)
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    if (H, W) == (2, 2):                                                # the single output: its ky = 2 and kx = 2 taps are all outside
        assert not got[2].any() and not got[:, 2].any() and got[:2, :2].any()


def test_on_the_byte_grid_the_terms_are_the_uint8_terms():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    dy = rng.normal(0, 1, (2, 3, 4, 8)).astype(f32)
    assert np.array_equal(ref.fc_terms(ref.byte_frames(u), dy), uref.fc_terms(u, dy))


# ----------------------------------------------------------------------------- the entry points' refusals
def test_every_refusal_of_the_entry_points_comes_before_any_hip_call(ssd):
    """No GPU here: a call that got past its checks would fail in HIP (SSD_ERR_HIP, -2) or touch the made-up addresses; every one of
    these returns SSD_ERR_INVALID (-1) with the argument named."""
    L = ssd.lib()
    B, H, W, C = 2, 6, 8, 8
    P = 0x7F0000001000                                                  # made-up, 16-byte aligned, never dereferenced
    need = L.ssd_first_conv_f32_train_workspace_bytes(B, H, W, C)
    assert need == L.ssd_first_conv_train_workspace_bytes(B, H, W, C) > 0       # the same formula as the uint8 block
    for shape in ((2, 128, 128, 32), (3, 10, 14, 24), (32, 640, 896, 32), (1, 2, 2, 4), (7, 32, 34, 64)):
        assert L.ssd_first_conv_f32_train_workspace_bytes(*shape) == L.ssd_first_conv_train_workspace_bytes(*shape) > 0, shape
    err = lambda: L.ssd_last_error()

    def fwd(b=B, h=H, ww=W, c=C, ip=P, wp=P + 0x1000, op=P + 0x2000):
        return L.ssd_first_conv_f32_train_forward(ip, b, h, ww, wp, c, op, None)

    def bwd(b=B, h=H, ww=W, c=C, ip=P, dyp=P + 0x1000, dwp=P + 0x2000, wsp=P + 0x3000, wsb=1 << 20):
        return L.ssd_first_conv_f32_train_backward(ip, dyp, b, h, ww, c, dwp, wsp, wsb, None)
    sized = L.ssd_first_conv_f32_train_workspace_bytes
    # the byte limit: B * H * W * 12 < 2^31 -- 312 frames of 640 x 896 pass the planner, 313 do not
    assert 312 * 640 * 896 * 12 < 2 ** 31 <= 313 * 640 * 896 * 12
    assert 2730 * 256 * 256 * 12 < 2 ** 31 <= 2731 * 256 * 256 * 12
    assert sized(312, 640, 896, 32) > 0 and sized(2730, 256, 256, 32) > 0
    for what, kw, word in (("odd H", dict(h=5), b"even"), ("odd W", dict(ww=7), b"even"),
                           ("Cout = 6", dict(c=6), b"Cout"), ("Cout = 68", dict(c=68), b"Cout"), ("Cout = 0", dict(c=0), b"Cout"),
                           ("B = 0", dict(b=0), b"positive"), ("H = 0", dict(h=0), b"positive"), ("W = -2", dict(ww=-2), b"positive"),
                           ("313 frames of 640 x 896", dict(b=313, h=640, ww=896), b"2^31"),
                           ("the first batch of 256 x 256 frames past 2^31 bytes", dict(b=2731, h=256, ww=256), b"2^31")):
        assert fwd(**kw) == -1 and word in err() and b"ssd_first_conv_f32_train_forward" in err(), what
        assert bwd(**kw) == -1 and word in err() and b"ssd_first_conv_f32_train_backward" in err(), what
        assert sized(kw.get("b", B), kw.get("h", H), kw.get("ww", W), kw.get("c", C)) == 0, what
    for kw in (dict(ip=None), dict(wp=None), dict(op=None)):
        assert fwd(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(ip=None), dict(dyp=None), dict(dwp=None), dict(wsp=None)):
        assert bwd(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(ip=P + 4), dict(ip=P + 8), dict(wp=P + 4), dict(op=P + 8)):
        assert fwd(**kw) == -1 and b"16-byte" in err(), kw
    for kw in (dict(ip=P + 4), dict(ip=P + 8), dict(dyp=P + 4), dict(dwp=P + 4), dict(wsp=P + 8)):
        assert bwd(**kw) == -1 and b"16-byte" in err(), kw
    assert bwd(wsb=need - 1) == -1 and b"workspace too small" in err()
    assert bwd(wsb=0) == -1 and b"workspace too small" in err()


# ----------------------------------------------------------------------------- train_calls on CPU tensors
@contextlib.contextmanager
def _library_not_called(ssd):
    L = ssd.lib()
    assert L.ssd_first_conv_f32_train_forward(None, 2, 6, 8, None, 8, None, None) == -1       # refused without a GPU: the sentinel
    sentinel = L.ssd_last_error()
    assert sentinel
    yield
    assert L.ssd_last_error() == sentinel


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _good(fn):
    return {"first_conv_f32_forward": lambda: dict(images=_z(2, 8, 12, 3), kernel=_z(3, 3, 3, 24), out=_z(2, 4, 6, 24)),
            "first_conv_f32_backward": lambda: dict(images=_z(2, 8, 12, 3), dy=_z(2, 4, 6, 24), dw=_z(3, 3, 3, 24))}[fn]()


def _spoil(t, kind):
    if kind == "shape":
        shape = list(t.shape)
        shape[1] += 1
        return torch.zeros(shape, dtype=t.dtype)
    if kind == "float64":
        return t.double()
    if kind == "uint8":
        return t.to(torch.uint8)
    assert kind == "strided"
    return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]


def test_the_planner_through_the_layer_is_the_raw_symbol(ssd):
    raw = ssd.lib().ssd_first_conv_f32_train_workspace_bytes(2, 8, 12, 24)
    assert raw > 0 and ssd.train_calls.first_conv_f32_workspace_bytes((2, 8, 12), 24) == raw
    assert ssd.train_calls.first_conv_f32_workspace_bytes(_z(2, 8, 12, 3), 24) == raw


@pytest.mark.parametrize("fn", ["first_conv_f32_forward", "first_conv_f32_backward"])
def test_correct_cpu_tensors_are_a_type_error(ssd, fn):
    with _library_not_called(ssd):
        with pytest.raises(TypeError, match="no CPU path"):
            getattr(ssd.train_calls, fn)(**_good(fn))


@pytest.mark.parametrize("fn,target,kind", [
    ("first_conv_f32_forward", "images", "uint8"), ("first_conv_f32_forward", "images", "float64"), ("first_conv_f32_forward", "images", "strided"),
    ("first_conv_f32_forward", "out", "shape"), ("first_conv_f32_forward", "kernel", "strided"), ("first_conv_f32_forward", "kernel", "float64"),
    ("first_conv_f32_backward", "images", "uint8"), ("first_conv_f32_backward", "images", "strided"), ("first_conv_f32_backward", "dy", "shape"),
    ("first_conv_f32_backward", "dy", "float64"), ("first_conv_f32_backward", "dw", "shape"), ("first_conv_f32_backward", "dw", "strided")])
def test_one_defect_is_a_value_error_that_names_the_argument(ssd, fn, target, kind):
    kw = _good(fn)
    kw[target] = _spoil(kw[target], kind)
    with _library_not_called(ssd):
        with pytest.raises(ValueError) as e:
            getattr(ssd.train_calls, fn)(**kw)
    assert target in str(e.value)


def test_a_workspace_that_is_not_uint8_is_a_value_error(ssd):
    with _library_not_called(ssd):
        with pytest.raises(ValueError, match="workspace"):
            ssd.train_calls.first_conv_f32_backward(workspace=_z(1 << 16), **_good("first_conv_f32_backward"))


# ----------------------------------------------------------------------------- the op and the modules
def test_first_conv_train_float_refuses_without_a_gpu(ssd):
    images = torch.zeros((1, 4, 4, 3))
    kernel = torch.zeros((3, 3, 3, 8))
    with pytest.raises(TypeError, match="GPU"):                         # CPU tensors
        ssd.first_conv_train_float(images, kernel)
    with pytest.raises(TypeError, match="float32"):                     # uint8 images are first_conv_train's
        ssd.first_conv_train_float(images.to(torch.uint8), kernel)
    with pytest.raises(TypeError, match="float32"):
        ssd.first_conv_train_float(images.double(), kernel)
    with pytest.raises(TypeError, match="float32"):
        ssd.first_conv_train_float(images, kernel.double())
    with pytest.raises(ValueError, match=r"\[3,3,3,Cout\]"):
        ssd.first_conv_train_float(images, torch.zeros((3, 3, 4, 8)))
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):               # channels first
        ssd.first_conv_train_float(torch.zeros((1, 3, 4, 4)), kernel)
    with pytest.raises(ValueError, match="even"):
        ssd.first_conv_train_float(torch.zeros((1, 3, 4, 3)), kernel)
    with pytest.raises(ValueError, match="Cout"):
        ssd.first_conv_train_float(images, torch.zeros((3, 3, 3, 6)))
    with pytest.raises(ValueError, match="Cout"):
        ssd.first_conv_train_float(images, torch.zeros((3, 3, 3, 68)))
    with pytest.raises(ValueError, match="no data gradient"):
        ssd.first_conv_train_float(images.clone().requires_grad_(), kernel)
    with pytest.raises(TypeError):
        ssd.first_conv_train_float(images.numpy(), kernel)
    with pytest.raises(TypeError, match="uint8"):                       # and first_conv_train keeps refusing floats
        ssd.first_conv_train(images, kernel)
