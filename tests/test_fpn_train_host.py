"""The TRAIN FPN's references and host side, without a GPU: tests/helpers/fpn_train_ref.py against finite differences of its own
forward, the zero-dilated form of the stride-2 data gradient, the initialiser's draw, and TrainableFPN's variable names."""
import numpy as np
import pytest

from helpers import fpn_train_ref as ref
from helpers import head_train_ref as href

f32 = np.float32


@pytest.mark.parametrize("k,stride,with_up", [(3, 2, False), (1, 1, False), (3, 1, False)])
def test_reference_gradients_agree_with_finite_differences(k, stride, with_up):
    """L = sum(conv(x, w) * dy) is linear in x and in w, so central differences are exact up to rounding: 1e-9 relative."""
    rng = np.random.default_rng(k * 10 + stride)
    B, H, W, Cin, Cout = 2, 5, 7, 3, 4
    x, w = rng.normal(0, 1, (B, H, W, Cin)), rng.normal(0, 1, (k, k, Cin, Cout))
    OH, OW = ref.out_hw(H, W, stride)
    dy = rng.normal(0, 1, (B, OH, OW, Cout))
    assert ref.conv(x, w, stride).shape == dy.shape
    (dx,), dw, _ = ref.conv_grads([x], w, [dy], stride)
    loss = lambda x_, w_: float((ref.conv(x_, w_, stride) * dy).sum())
    h = 1e-3
    for arr, grad, which in ((x, dx, 0), (w, dw, 1)):
        for _ in range(12):
            idx = tuple(rng.integers(0, s) for s in arr.shape)
            e = np.zeros(arr.shape)
            e[idx] = h
            fd = (loss(x + e, w) - loss(x - e, w)) / (2 * h) if which == 0 else (loss(x, w + e) - loss(x, w - e)) / (2 * h)
            assert abs(fd - grad[idx]) <= 1e-9 * max(1.0, abs(grad[idx])), (which, idx)


def test_explicit_pad_forward_is_the_valid_convolution_of_the_padded_input():
    """conv2d_same stride 2 (layer_utils.py:25-43): pad 1 before and after, then 'valid': 5 x 7 -> 3 x 4, 6 x 8 -> 3 x 4."""
    rng = np.random.default_rng(1)
    for H, W in ((5, 7), (6, 8), (1, 1), (2, 2)):
        x, w = rng.integers(-3, 4, (1, H, W, 2)).astype(np.float64), rng.integers(-2, 3, (3, 3, 2, 3)).astype(np.float64)
        p = np.zeros((1, H + 2, W + 2, 2))
        p[:, 1:-1, 1:-1] = x
        OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        want = np.zeros((1, OH, OW, 3))
        for oy in range(OH):
            for ox in range(OW):
                want[0, oy, ox] = np.einsum("hwi,hwio->o", p[0, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3], w)
        assert (OH, OW) == ref.out_hw(H, W, 2) and np.array_equal(ref.conv(x, w, 2), want)


@pytest.mark.parametrize("H,W", [(5, 7), (6, 8), (1, 1), (2, 2)])
def test_dilation_identity_holds_exactly_on_integers(H, W):
    """dx of the stride-2 convolution == conv3x3_same(D, w'), D the zero-dilated dy, w' the rotated transposed kernel."""
    rng = np.random.default_rng(H * 10 + W)
    B, Cin, Cout = 2, 8, 5
    x = rng.integers(-3, 4, (B, H, W, Cin)).astype(f32)
    w = rng.integers(-2, 3, (3, 3, Cin, Cout)).astype(f32)
    OH, OW = ref.out_hw(H, W, 2)
    dy = rng.integers(-3, 4, (B, OH, OW, Cout)).astype(f32)
    (dx,), _, _ = ref.conv_grads([x], w, [dy], 2)
    D = ref.dilate(dy, H, W)
    assert D.sum() == dy.sum() and np.array_equal(D[:, ::2, ::2], dy)
    assert np.array_equal(ref.conv(D, href.rotated_transposed(w), 1), dx) and np.abs(dx).max() > 0


def test_merge_restatement_on_a_hand_case():
    g = np.arange(16, dtype=f32).reshape(1, 4, 4, 1)
    base = np.full((1, 2, 2, 1), 100, f32)
    assert np.array_equal(ref.merge_f32(g, base)[0, :, :, 0], [[110, 118], [142, 150]])
    gate = np.array([[1, -0.0], [np.nan, 2]], f32).reshape(1, 2, 2, 1)
    assert np.array_equal(ref.merge_f32(g, None, gate)[0, :, :, 0], [[10, 0], [0, 50]])
    assert np.array_equal(ref.merge_f32(base, base, gate, same_size=True)[0, :, :, 0], [[200, 100], [100, 200]])


def test_initialiser_draw_has_the_stated_variance():
    import ssd_amd
    for shape in ((3, 3, 256, 256), (1, 1, 116, 256)):
        a = ssd_amd.variance_scaling_draw(np.random.default_rng(3), shape)
        fan_in = shape[0] * shape[1] * shape[2]
        s = np.sqrt(1.0 / fan_in) / 0.87962566103423978
        assert a.dtype == f32 and a.shape == shape and np.abs(a).max() <= 2 * s * (1 + 1e-6)
        n = a.size
        # the sample variance of n draws of variance v and kurtosis < 3 has standard error < v * sqrt(2 / n): 6 sigma
        assert abs(a.astype(np.float64).var() * fan_in - 1.0) <= 6 * np.sqrt(2.0 / n)
        assert abs(a.astype(np.float64).mean()) <= 6 * np.sqrt(1.0 / fan_in / n)
    b = ssd_amd.variance_scaling_draw(np.random.default_rng(3), (1, 1, 116, 256))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_trainable_fpn_names_are_the_fpn_subset(backbone):
    import ssd_amd
    params = {"backbone": backbone, "depth_multiplier": 1.0, "num_classes": 80}
    shapes = ssd_amd.variable_shapes(params)
    want = [k for k in shapes if k.startswith("fpn/")]
    assert len(want) == 8 + 5 * 4 and list(ssd_amd.fpn_variable_shapes(params)) == want
    m = ssd_amd.TrainableFPN(params, {}, seed=5)                        # the warm-start case: no fpn/* in the weights
    stats = [k for k in want if k.rsplit("/", 1)[1] in ("moving_mean", "moving_variance")]
    assert list(m.statistics()) == stats and list(m.named_variables()) == [k for k in want if k not in stats]
    for k in want:
        v = m.variable(k).detach().numpy()
        assert tuple(v.shape) == tuple(shapes[k])
        leaf = k.rsplit("/", 1)[1]
        if leaf in ("gamma", "moving_variance"):
            assert np.all(v == 1)
        elif leaf in ("beta", "moving_mean"):
            assert np.all(v == 0)
        else:
            assert abs(v.astype(np.float64).var() * np.prod(shapes[k][:3]) - 1.0) < 0.05
    W = ssd_amd.synthetic_weights(params, seed=2)
    m2 = ssd_amd.TrainableFPN(params, W)
    assert all(np.array_equal(m2.variable(k).detach().numpy(), W[k]) for k in want)
    with pytest.raises(ValueError):
        ssd_amd.TrainableFPN(params, {"fpn/p3/kernel": np.zeros((3, 3, 8, 256), f32)})
