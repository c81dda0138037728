"""The TRAIN backbone on the CPU (include/ssd_hip.h, "the TRAIN backbone"): the header's restatements of the depthwise convolution's
two gradients against torch autograd of the grouped convolution, exactly, on small integers; the float32 operation sequence of the
batch norm with ReLU6 on a hand case; the backbone's variable list."""
import numpy as np
import pytest

from helpers import backbone_train_ref as ref
from conftest import TINY_PARAMS

f32 = np.float32
CASES = [(6, 8, 2), (5, 7, 2), (5, 7, 1), (1, 1, 1), (1, 1, 2), (2, 2, 1), (2, 2, 2)]


def _integers(h, w, stride, C=8, B=2):
    rng = np.random.default_rng(h * 100 + w * 10 + stride)
    x = rng.integers(-3, 4, (B, h, w, C)).astype(f32)
    k = rng.integers(-2, 3, (3, 3, C, 1)).astype(f32)
    dy = rng.integers(-3, 4, (B,) + ref.dw_out_hw(h, w, stride) + (C,)).astype(f32)
    return x, k, dy


@pytest.mark.parametrize("h,w,stride", CASES)
def test_data_gradient_is_the_depthwise_convolution_of_E_with_the_flipped_kernel(oracle_ops, h, w, stride):
    """dx = depthwise3x3(E, flip(w), stride 1), E zero except E[b, s*oy+1-p, s*ox+1-p] = dy[b,oy,ox]: equal to autograd of the
    grouped convolution with TF 'SAME' padding, exactly, on small integers; the forward is the oracle's too."""
    x, k, dy = _integers(h, w, stride)
    y, dx, _ = ref.torch_depthwise(x, k, stride, dy)
    assert np.array_equal(oracle_ops.depthwise3x3(x, k, stride).astype(np.float64), y)
    E = ref.dilate_E(dy, h, w, stride)
    assert E.shape == x.shape and np.count_nonzero(E) == np.count_nonzero(dy)
    if stride == 1:
        assert np.array_equal(E, dy)
    got = oracle_ops.depthwise3x3(E, ref.flip(k), 1)
    assert np.array_equal(got.astype(np.float64), dx) and np.abs(dx).max() > 0


@pytest.mark.parametrize("h,w,stride", CASES)
def test_weight_gradient_restatement_is_autograds(h, w, stride):
    x, k, dy = _integers(h, w, stride)
    _, _, dw = ref.torch_depthwise(x, k, stride, dy)
    terms = ref.dw_terms(x, dy, stride)
    assert terms.shape == (dy.size // dy.shape[3], 9, x.shape[3])
    assert np.array_equal(terms.sum(0).reshape(3, 3, -1, 1), dw) and np.abs(dw).max() > 0


def test_same_padding_of_the_cases():
    assert [ref.same(n, 2) for n in (5, 6, 7, 8, 1, 2)] == [(3, 1), (3, 0), (4, 1), (4, 0), (1, 1), (1, 0)]
    assert [ref.same(n, 1) for n in (1, 2, 7)] == [(1, 1), (2, 1), (7, 1)]


def test_batch_norm_relu6_float32_sequence_on_a_hand_case():
    """gamma 2, invstd 1/2 (sf = 1), mean 0, beta 0: y = x.  y exactly 0, exactly 6, just under 6, NaN, negative, above 6, inside.
    With dbeta = R and dgamma = 2 R: dx = sf * ((g - 1) - (x / 2) * 2) = g - 1 - x."""
    below6 = np.nextafter(f32(6), f32(0))
    x = np.array([0.0, 6.0, below6, np.nan, -1.0, 7.0, 3.0], f32).reshape(7, 1)
    dy = np.array([10, 20, 30, 40, 50, 60, 70], f32).reshape(7, 1)
    one = np.ones(1, f32)
    ypre, out, dx = ref.bn_act_f32(x, 2 * one, 0 * one, 0 * one, None, "relu6", dy, dgamma=14 * one, dbeta=7 * one, invstd=0.5 * one)
    assert np.array_equal(ypre[[0, 1, 2, 4, 5, 6], 0], x[[0, 1, 2, 4, 5, 6], 0]) and np.isnan(ypre[3, 0])
    assert np.array_equal(out[:, 0], np.array([0, 6, below6, 0, 0, 6, 3], f32))
    g = np.array([0, 0, 30, 0, 0, 0, 70], f32)
    want = g - f32(1) - x[:, 0]
    assert np.array_equal(dx[[0, 1, 2, 4, 5, 6], 0], want[[0, 1, 2, 4, 5, 6]]) and np.isnan(dx[3, 0])
    # ReLU on the same data: 6 and 7 pass, their gates are open
    _, out1, dx1 = ref.bn_act_f32(x, 2 * one, 0 * one, 0 * one, None, "relu", dy, dgamma=14 * one, dbeta=7 * one, invstd=0.5 * one)
    assert np.array_equal(out1[:, 0], np.array([0, 6, below6, 0, 0, 7, 3], f32))
    g1 = np.array([0, 20, 30, 0, 0, 60, 70], f32)
    assert np.array_equal(dx1[[0, 1, 2, 4, 5, 6], 0], (g1 - f32(1) - x[:, 0])[[0, 1, 2, 4, 5, 6]])
    # the same sequence element by element in float32 scalars, on statistics that round
    rng = np.random.default_rng(3)
    xs, dys = rng.normal(1, 3, (50, 3)).astype(f32), rng.normal(0, 1, (50, 3)).astype(f32)
    gamma, beta, mean, var = (rng.uniform(0.5, 1.5, 3).astype(f32) for _ in range(4))
    dgamma, dbeta = rng.normal(0, 5, 3).astype(f32), rng.normal(0, 5, 3).astype(f32)
    ypre, out, dx = ref.bn_act_f32(xs, gamma, beta, mean, var, "relu6", dys, dgamma=dgamma, dbeta=dbeta)
    assert (ypre >= 6).any() and (ypre <= 0).any() and ((ypre > 0) & (ypre < 6)).any()
    R = f32(50)
    for r in range(50):
        for c in range(3):
            invstd = f32(1) / np.sqrt(f32(var[c] + f32(ref.EPS)))
            t = f32(xs[r, c] - mean[c])
            sf = f32(gamma[c] * invstd)
            y = f32(f32(t * sf) + beta[c])
            v = y if y > 0 else f32(0)
            v = v if v < 6 else f32(6)
            g = dys[r, c] if (y > 0 and y < 6) else f32(0)
            d = f32(sf * f32(f32(g - f32(dbeta[c] / R)) - f32(f32(t * invstd) * f32(dgamma[c] / R))))
            assert out[r, c] == v and dx[r, c] == d, (r, c)


def test_mobilenet_variable_shapes_is_the_mobilenet_subset(ssd):
    shapes = ssd.variable_shapes(TINY_PARAMS)
    sub = ssd.mobilenet_variable_shapes(TINY_PARAMS)
    assert sub == {k: v for k, v in shapes.items() if k.startswith("MobilenetV1/")} and list(sub) == [k for k in shapes if k in sub]
    assert len(sub) == 5 + 13 * 10 and not any(k.startswith(("fpn/", "box_net/", "class_net/")) for k in sub)
    assert len(sub) + len(ssd.fpn_variable_shapes(TINY_PARAMS)) + len(ssd.head_variable_shapes(TINY_PARAMS)) == len(shapes)
    with pytest.raises(ValueError):
        ssd.mobilenet_variable_shapes(dict(TINY_PARAMS, backbone="shufflenet"))
    W = ssd.synthetic_weights(TINY_PARAMS, seed=1)
    with pytest.raises(ValueError, match="backbone"):
        ssd.TrainableMobileNet(dict(TINY_PARAMS, backbone="shufflenet"), W)
    with pytest.raises(ValueError, match="depth_multiplier"):
        ssd.TrainableMobileNet(dict(TINY_PARAMS, depth_multiplier=2.0), W)
    with pytest.raises(KeyError):
        ssd.TrainableMobileNet(TINY_PARAMS, {k: v for k, v in W.items() if k != "MobilenetV1/Conv2d_7_pointwise/weights"})
    m = ssd.TrainableMobileNet(TINY_PARAMS, W)
    assert len(m.named_variables()) == 78 and len(m.statistics()) == 52
    assert sorted(m.frozen_variables()) == sorted(k for k in sub if k.startswith("MobilenetV1/Conv2d_0/"))
