"""The TRAIN first convolution on the CPU (include/ssd_hip.h, "the TRAIN first convolution"): the premises of the GPU tests -- the
256 pixel values against the oracle's preprocess and their grid, the weight gradient's restatement against torch autograd, exactly
-- and the refusals of first_conv_train that need no GPU."""
import numpy as np
import pytest

from helpers import first_conv_train_ref as ref

f32 = np.float32
f64 = np.float64


def test_the_256_pixel_values_are_the_oracles_and_lie_on_the_2_to_the_minus_24_grid(oracle_ops):
    """p(u) in numpy float32 equals preprocess(u), and p * 2^24 is an integer for every byte: every p is a float32 in [-1, 1] that
    is either at least 1/2 in magnitude (the float32 spacing there is 2^-24 or 2^-23) or the exact difference of a multiple of
    2^-24 and 1 (|2v - 1| < 1/2 means 1/2 < 2v < 3/2: 2v is a multiple of 2^-24 and the subtraction is exact by Sterbenz).  The
    exactness test of the weight gradient rests on this."""
    p = ref.pixel_table()
    want = oracle_ops.preprocess(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)).reshape(256)
    assert p.dtype == f32 and np.array_equal(p.view(np.int32), want.view(np.int32))
    assert p[0] == -1 and p[255] == 1 and np.all(np.diff(p) > 0) and np.all(np.abs(p) <= 1)
    scaled = p.astype(f64) * 2.0 ** 24
    assert np.array_equal(scaled, np.round(scaled))


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (6, 4)])
def test_the_weight_gradients_restatement_is_torch_autograd_exactly(H, W):
    """sum over the rows of fc_terms == the gradient of the float64 stride-2 convolution of the frame padded by one row and column
    at the bottom and right, with integer dy in [-8, 8]: every term is a multiple of 2^-24 below 2^3, so both sums are exact."""
    rng = np.random.default_rng(H * 10 + W)
    B, Cout = 2, 8
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    dy = rng.integers(-8, 9, (B, H // 2, W // 2, Cout)).astype(f32)
    terms = ref.fc_terms(images, dy)
    assert terms.shape == (B * (H // 2) * (W // 2), 27, Cout)
    units = terms * 2.0 ** 24
    assert np.array_equal(units, np.round(units)) and np.abs(units).sum(0).max() < 2.0 ** 53
    got = terms.sum(0).reshape(3, 3, 3, Cout)
    want = ref.torch_dw(images, dy)
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    if (H, W) == (2, 2):                                                # the single output: its ky = 2 and kx = 2 taps are all outside
        assert not got[2].any() and not got[:, 2].any() and got[:2, :2].any()


def test_first_conv_train_refuses_without_a_gpu():
    import torch
    import ssd_amd
    images = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    kernel = torch.zeros((3, 3, 3, 8))
    with pytest.raises(TypeError, match="GPU"):                         # CPU tensors
        ssd_amd.first_conv_train(images, kernel)
    with pytest.raises(TypeError, match="uint8"):                       # float images
        ssd_amd.first_conv_train(images.float(), kernel)
    with pytest.raises(ValueError, match=r"\[3,3,3,Cout\]"):
        ssd_amd.first_conv_train(images, torch.zeros((3, 3, 4, 8)))
    with pytest.raises(ValueError, match="even"):
        ssd_amd.first_conv_train(torch.zeros((1, 3, 4, 3), dtype=torch.uint8), kernel)
    with pytest.raises(ValueError, match="Cout"):
        ssd_amd.first_conv_train(images, torch.zeros((3, 3, 3, 6)))
    with pytest.raises(TypeError):
        ssd_amd.first_conv_train(images.numpy(), kernel)
