"""The TRAIN ShuffleNet on the CPU (include/ssd_hip.h, "the TRAIN ShuffleNet"): the restatements of helpers/shufflenet_train_ref.py
against the oracle and torch autograd, the backbone's variable list, the checks of ssd.train_calls on CPU tensors, and every new
entry point's refusals through the loaded library -- they come before any HIP call, so they need no GPU."""
import ctypes

import numpy as np
import pytest

from helpers import shufflenet_train_ref as ref
from conftest import TINY_PARAMS

f32 = np.float32
SN_PARAMS = dict(TINY_PARAMS, backbone="shufflenet")


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ----------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("D", [1, 2, 58])
def test_the_shuffles_transpose_after_the_oracles_shuffle_is_the_identity(oracle_ops, D):
    rng = np.random.default_rng(D)
    x, y = rng.normal(0, 1, (7, D)).astype(f32), rng.normal(0, 1, (7, D)).astype(f32)
    xo, yo = oracle_ops.concat_shuffle_split(x, y)
    z = np.stack([x, y], axis=-1).reshape(7, 2 * D)                       # z[2i] = x[i], z[2i+1] = y[i]
    assert np.array_equal(xo, z[:, :D]) and np.array_equal(yo, z[:, D:])
    bx, by = ref.shuffle_transpose(xo, yo)
    assert np.array_equal(_bits(bx), _bits(x)) and np.array_equal(_bits(by), _bits(y))


@pytest.mark.parametrize("h,w", [(4, 6), (8, 8), (2, 2)])
def test_the_max_pool_restatement_is_autograds_on_tie_free_data(oracle_ops, h, w):
    """Distinct values (a permutation), integer dy: no window has a tie and the order of the additions cannot matter."""
    rng = np.random.default_rng(h * 10 + w)
    x = rng.permutation(2 * h * w * 8).astype(f32).reshape(2, h, w, 8) - f32(h * w * 8)
    dy = rng.integers(-4, 5, (2, h // 2, w // 2, 8)).astype(f32)
    y, dx = ref.torch_maxpool(x, dy)
    assert np.array_equal(ref.maxpool_forward(x).astype(np.float64), y) and np.array_equal(oracle_ops.maxpool3x3s2(x).astype(np.float64), y)
    got = ref.maxpool_grad(x, dy)
    assert np.array_equal(got.astype(np.float64), dx) and np.abs(dx).max() > 0
    assert got.sum() == dy.sum()                                          # every window gave its gradient to exactly one tap


def test_the_max_pool_tie_rule_on_hand_built_windows():
    """4 x 4, one channel per case: windows (0,0) = rows 0..2 x columns 0..2, (0,1) = columns 2..3, (1,0) = rows 2..3, (1,1) = [2:,2:]."""
    x = np.zeros((1, 4, 4, 4), f32)
    dy = np.array([[1, 2], [4, 8]], f32).reshape(1, 2, 2, 1).repeat(4, 3)
    x[0, :, :, 0] = 5.0                                                   # all equal: the first tap of every window wins
    x[0, :, :, 1] = np.nan                                                # all NaN: nobody wins
    x[0, :, :, 2] = np.nan
    x[0, 1, 1, 2] = -np.inf                                               # the only number of window (0,0) is -inf = the output: it wins
    x[0, :, :, 3] = [[0, 0, 0, 0], [0, 7, 7, 0], [0, 7, 9, 0], [0, 0, 0, 0]]       # (2,2) wins all four windows; 7 ties never do
    dx = ref.maxpool_grad(x, dy)
    want0 = np.zeros((4, 4), f32)
    want0[0, 0], want0[0, 2], want0[2, 0], want0[2, 2] = 1, 2, 4, 8
    assert np.array_equal(dx[0, :, :, 0], want0)
    assert np.array_equal(dx[0, :, :, 1], np.zeros((4, 4), f32))
    want2 = np.zeros((4, 4), f32)
    want2[1, 1] = 1
    assert np.array_equal(dx[0, :, :, 2], want2)
    want3 = np.zeros((4, 4), f32)
    want3[2, 2] = 15
    assert np.array_equal(dx[0, :, :, 3], want3)
    out = ref.maxpool_forward(x)
    assert np.all(out[0, :, :, 0] == 5) and np.all(out[0, :, :, 1] == -np.inf) and np.all(out[0, :, :, 3] == 9)


def test_the_batch_norm_without_activation_is_the_relu_sequence_with_every_gate_open():
    from helpers import backbone_train_ref as bref
    rng = np.random.default_rng(5)
    x, dy = rng.normal(5, 1, (40, 3)).astype(f32), rng.normal(0, 1, (40, 3)).astype(f32)
    gamma, mean, var = (rng.uniform(0.5, 1.5, 3).astype(f32) for _ in range(3))
    beta = np.full(3, 2, f32)                                             # y > 0 everywhere: ReLU is the identity and its gate open
    dgamma, dbeta = rng.normal(0, 5, 3).astype(f32), rng.normal(0, 5, 3).astype(f32)
    invstd = bref.href.invstd_f32(var)
    ypre, out, dx = bref.bn_act_f32(x, gamma, beta, mean, var, "relu", dy, dgamma=dgamma, dbeta=dbeta)
    assert (ypre > 0).all()
    y, dx2 = ref.bn_none_f32(x, gamma, beta, mean, invstd, dy, dgamma, dbeta)
    assert np.array_equal(_bits(y), _bits(out)) and np.array_equal(_bits(dx2), _bits(dx))
    # and where y is negative the value passes, the gradient too
    y, dx3 = ref.bn_none_f32(-x, gamma, -beta, -mean, invstd, dy, dgamma, dbeta)
    assert (y < 0).all() and np.array_equal(_bits(y), _bits(-out))


# ----------------------------------------------------------------------------- the variables
@pytest.mark.parametrize("depth", [0.5, 1.0, 1.5])
def test_shufflenet_variable_counts(ssd, depth):
    params = dict(SN_PARAMS, depth_multiplier=depth)
    shapes = ssd.variable_shapes(params)
    sub = ssd.shufflenet_variable_shapes(params)
    assert sub == {k: v for k, v in shapes.items() if k.startswith("ShuffleNetV2/")} and list(sub) == [k for k in shapes if k in sub]
    assert len(sub) == 280 and sum(k.endswith(("moving_mean", "moving_variance")) for k in sub) == 112
    assert len(sub) + len(ssd.fpn_variable_shapes(params)) + len(ssd.head_variable_shapes(params)) == len(shapes)
    W = ssd.synthetic_weights(params, seed=1)
    m = ssd.TrainableShuffleNet(params, W)
    assert (len(m.named_variables()), len(m.statistics()), len(m.frozen_variables())) == (165, 110, 5)
    assert sorted(m.frozen_variables()) == sorted(k for k in sub if k.startswith("ShuffleNetV2/Conv1/"))
    m = ssd.TrainableShuffleNet(params, W, train_first=True)
    assert (len(m.named_variables()), len(m.statistics()), len(m.frozen_variables())) == (168, 112, 0)
    assert list(m.named_variables()) + list(m.statistics()) != [] and set(m.named_variables()) | set(m.statistics()) == set(sub)


def test_shufflenet_module_refuses_what_it_cannot_train(ssd):
    W = ssd.synthetic_weights(SN_PARAMS, seed=1)
    with pytest.raises(ValueError, match="depth_multiplier"):
        ssd.TrainableShuffleNet(dict(SN_PARAMS, depth_multiplier=2.0), ssd.synthetic_weights(dict(SN_PARAMS, depth_multiplier=2.0), seed=1))
    with pytest.raises(ValueError, match="backbone"):
        ssd.TrainableShuffleNet(TINY_PARAMS, W)
    with pytest.raises(ValueError, match="backbone"):
        ssd.shufflenet_variable_shapes(TINY_PARAMS)
    with pytest.raises(KeyError):
        ssd.TrainableShuffleNet(SN_PARAMS, {k: v for k, v in W.items() if k != "ShuffleNetV2/Stage3/unit_5/depthwise/depthwise_weights"})
    with pytest.raises(KeyError):
        ssd.TrainableShuffleNet(SN_PARAMS, {k: v for k, v in W.items() if k != "ShuffleNetV2/Conv1/weights"})
    with pytest.raises(ValueError, match="backbone"):                     # and MobileNet's module keeps its refusal
        ssd.TrainableMobileNet(SN_PARAMS, W)


# ----------------------------------------------------------------------------- train_calls on CPU tensors
def test_train_calls_checks_run_on_cpu_tensors(ssd):
    import torch
    calls = ssd.train_calls
    z = lambda *s: torch.zeros(s)
    x, y = z(3, 5, 6), z(3, 5, 6)
    with pytest.raises(ValueError, match="y"):
        calls.shuffle(x, z(3, 5, 8), z(3, 5, 6), z(3, 5, 6))
    with pytest.raises(ValueError, match="yo"):
        calls.shuffle(x, y, z(3, 5, 6), z(3, 5, 6).double())
    with pytest.raises(ValueError, match="out"):
        calls.concat(x, y, z(3, 5, 6))
    with pytest.raises(ValueError, match="g"):
        calls.split(z(3, 5, 6), z(3, 5, 6), z(3, 5, 6))
    with pytest.raises(ValueError, match="dy"):
        calls.maxpool_backward(z(2, 4, 6, 8), z(2, 4, 6, 8), z(2, 4, 6, 8))
    with pytest.raises(TypeError, match="GPU"):                           # every shape is right: only the device is left to refuse
        calls.shuffle(x, y, z(3, 5, 6), z(3, 5, 6))
    with pytest.raises(TypeError, match="GPU"):
        calls.concat(x, y, z(3, 5, 12))
    with pytest.raises(TypeError, match="GPU"):
        calls.split(z(3, 5, 12), x, y)
    with pytest.raises(TypeError, match="GPU"):
        calls.maxpool_backward(z(2, 4, 6, 8), z(2, 2, 3, 8), z(2, 4, 6, 8))
    # the entries: the old ones refuse what they refused, "none" only with sn_bn
    k = z(3, 3, 6, 1)
    with pytest.raises(ValueError, match="entry"):
        calls.depthwise_forward(z(2, 4, 4, 6), k, z(2, 4, 4, 6), entry="sn")
    with pytest.raises(TypeError, match="GPU"):
        calls.depthwise_forward(z(2, 4, 4, 6), k, z(2, 4, 4, 6), entry="sn_depthwise")
    vec = [z(6)]
    for entry, act in (("bn_act", "none"), ("bn_act", "tanh"), ("bn_relu", "none"), ("sn_bn", "tanh"), ("sn", "relu")):
        with pytest.raises(ValueError, match="entry"):
            calls.bn_forward([z(10, 6)], [z(10, 6)], vec, vec, True, 1e-3, 0.007, vec, vec, vec, vec, vec, act=act, entry=entry)
    with pytest.raises(TypeError, match="GPU"):
        calls.bn_forward([z(10, 6)], [z(10, 6)], vec, vec, True, 1e-3, 0.007, vec, vec, vec, vec, vec, act="none", entry="sn_bn")
    w = z(1, 1, 6, 10)
    with pytest.raises(ValueError, match="bias"):
        calls.conv_forward([z(2, 4, 4, 6)], w, [z(2, 4, 4, 10)], bias=z(10), entry="sn_pointwise")
    with pytest.raises(ValueError, match="entry"):
        calls.conv_forward([z(2, 4, 4, 6)], z(3, 3, 6, 10), [z(2, 4, 4, 10)], entry="sn_pointwise")
    with pytest.raises(ValueError, match="forward"):
        calls.conv_forward([z(2, 4, 4, 8)], z(1, 1, 8, 10), [z(2, 4, 4, 10)], entry="pointwise")
    with pytest.raises(TypeError, match="GPU"):
        calls.conv_forward([z(2, 4, 4, 6)], w, [z(2, 4, 4, 10)], entry="sn_pointwise")
    with pytest.raises(ValueError, match="act"):
        ssd.batch_norm_act(z(10, 6), z(6), z(6), z(6), z(6), training=True, act="tanh")
    # the planners need no GPU either
    assert calls.depthwise_workspace_bytes((2, 16, 16, 58), 1, entry="sn_depthwise") > 0
    assert calls.depthwise_workspace_bytes((2, 16, 16, 58), 1) == 0
    assert calls.conv_workspace_bytes([(5, 7)], 2, 58, 58, 1, entry="sn_pointwise") > 0
    assert calls.conv_workspace_bytes([(5, 7)], 2, 58, 58, 1, entry="pointwise") == 0


# ----------------------------------------------------------------------------- refusals through the library
def _aligned(nbytes):
    """A host buffer and a 16-byte aligned address inside it: the refusals below never reach a kernel, so no byte of it is read."""
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_every_new_entry_point_refuses_bad_arguments_before_any_hip_call(ssd):
    L = ssd.lib()
    B, H, W = 2, 6, 8
    keep, p = _aligned(1 << 20)
    err = lambda: L.ssd_last_error().decode()

    # depthwise: odd C, C > 1024 backward, misaligned, short workspace
    assert L.ssd_sn_depthwise_train_forward(p, B, H, W, 7, p, 1, p, None) == -1 and "C must be even" in err()
    assert L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, 7, 1) == 0
    assert L.ssd_sn_depthwise_train_backward(p, p, B, H, W, 7, p, 1, p, p, p, 1 << 20, None) == -1 and "C must be even" in err()
    assert L.ssd_sn_depthwise_train_backward(p, p, B, H, W, 1026, p, 1, p, p, p, 1 << 20, None) == -1 and "1024" in err()
    assert L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, 1026, 1) == 0
    assert L.ssd_sn_depthwise_train_forward(p + 8, B, H, W, 58, p, 1, p, None) == -1 and "16-byte" in err()
    need = L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, 58, 1)
    rpp, slab_rows, slabs = ref.href.slab_plan([B * H * W], 58)          # G = ceil(58 / 4) = 15 quads
    assert (rpp, slab_rows, slabs) == (17, 136, 1) and need == ref.href.al256(slabs * 9 * 58 * 8)
    assert L.ssd_sn_depthwise_train_backward(p, p, B, H, W, 58, p, 1, p, p, p, need - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_depthwise_train_backward(p, p + 4, B, H, W, 58, p, 1, p, p, p, need, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_depthwise_train_forward(p, B, H, W, 58, p, 3, p, None) == -1 and "stride" in err()
    # for C % 4 == 0 the planner is the old one
    assert L.ssd_sn_depthwise_train_workspace_bytes(B, H, W, 8, 1) == L.ssd_depthwise_train_workspace_bytes(B, H, W, 8, 1) > 0
    assert L.ssd_depthwise_train_workspace_bytes(B, H, W, 58, 1) == 0      # and the old entry point keeps its refusal

    # pointwise: odd Cin / Cout, too wide, short workspace, misaligned dx
    CL = ssd._lib.SsdConvLevel
    lv = lambda x=p, dy=p, out=p: (CL * 1)(CL(H, W, x, dy, out))
    assert L.ssd_sn_pointwise_train_workspace_bytes(lv(), 1, B, 7, 10) == 0 and L.ssd_sn_pointwise_train_workspace_bytes(lv(), 1, B, 6, 9) == 0
    assert L.ssd_sn_pointwise_train_workspace_bytes(lv(), 1, B, 4098, 10) == 0
    assert L.ssd_sn_pointwise_train_forward(lv(), 1, B, 7, 10, p, p, 1 << 20, None) == -1 and "Cin" in err()
    assert L.ssd_sn_pointwise_train_backward(lv(), 1, B, 6, 9, p, p, p, 1 << 20, None) == -1 and "Cout" in err()
    assert L.ssd_sn_pointwise_train_forward(lv(), 1, B, 4098, 10, p, p, 1 << 20, None) == -1 and "4096" in err()
    pneed = L.ssd_sn_pointwise_train_workspace_bytes(lv(), 1, B, 58, 58)
    assert 0 < pneed <= 1 << 20
    assert L.ssd_sn_pointwise_train_forward(lv(), 1, B, 58, 58, p, p, pneed - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_pointwise_train_backward(lv(), 1, B, 58, 58, p, p, p, pneed - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_pointwise_train_backward(lv(out=p + 4), 1, B, 58, 58, p, p, p, pneed, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_pointwise_train_workspace_bytes(lv(), 1, B, 8, 16) == L.ssd_pointwise_train_workspace_bytes(lv(), 1, B, 8, 16) > 0
    assert L.ssd_pointwise_train_workspace_bytes(lv(), 1, B, 6, 16) == 0

    # batch norm: act 3, misaligned, short workspace; the old pair still refuses act 0
    Lv = ssd._lib.SsdBnLevel
    rows, C = B * H * W, 58
    bl = lambda x=p: (Lv * 1)(Lv(rows, x, p, p, *([p] * 9)))
    bneed = L.ssd_bn_relu_train_workspace_bytes(bl(), 1, C)
    assert 0 < bneed <= 1 << 20
    assert L.ssd_sn_bn_train_forward(bl(), 1, C, 3, 1, 1e-3, 0.007, p, bneed, None) == -1 and "act" in err() and "SSD_ACT_NONE" in err()
    assert L.ssd_sn_bn_train_backward(bl(), 1, C, 3, p, bneed, None) == -1 and "act" in err()
    assert L.ssd_sn_bn_train_forward(bl(x=p + 4), 1, C, 0, 1, 1e-3, 0.007, p, bneed, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_bn_train_forward(bl(), 1, C, 0, 1, 1e-3, 0.007, p, bneed - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_bn_train_backward(bl(), 1, C, 0, p, bneed - 1, None) == -1 and "workspace too small" in err()
    assert L.ssd_sn_bn_train_forward(bl(), 1, 1025, 0, 1, 1e-3, 0.007, p, 1 << 20, None) == -1 and "1024" in err()
    assert L.ssd_bn_act_train_forward(bl(), 1, C, 0, 1, 1e-3, 0.007, p, bneed, None) == -1 and "act" in err()
    assert L.ssd_bn_act_train_backward(bl(), 1, C, 0, p, bneed, None) == -1 and "act" in err()

    # shuffle, concat, split: rows < 1, D < 1, null, misaligned, overlap
    q = p + 4096
    for rc in (L.ssd_sn_shuffle_train(p, q, 0, 4, 0, q + 4096, q + 8192, None), L.ssd_sn_concat_train(p, q, 0, 4, q + 4096, None),
               L.ssd_sn_split_train(p, 0, 4, q, q + 4096, None)):
        assert rc == -1 and "rows" in err()
    for rc in (L.ssd_sn_shuffle_train(p, q, 3, 0, 0, q + 4096, q + 8192, None), L.ssd_sn_concat_train(p, q, 3, 0, q + 4096, None),
               L.ssd_sn_split_train(p, 3, 0, q, q + 4096, None)):
        assert rc == -1 and "D" in err()
    assert L.ssd_sn_shuffle_train(p, None, 3, 4, 0, q + 4096, q + 8192, None) == -1 and "null" in err()
    assert L.ssd_sn_shuffle_train(p, q + 4, 3, 4, 1, q + 4096, q + 8192, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_concat_train(p, q, 3, 4, q + 4100, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_split_train(p + 8, 3, 4, q, q + 4096, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_shuffle_train(p, q, 3, 4, 0, p + 32, q + 8192, None) == -1 and "overlap" in err()      # xo inside x's 48 bytes
    assert L.ssd_sn_shuffle_train(p, q, 3, 4, 0, q + 4096, q + 4096 + 32, None) == -1 and "overlap" in err()
    assert L.ssd_sn_concat_train(p, q, 3, 4, p + 16, None) == -1 and "overlap" in err()
    assert L.ssd_sn_split_train(p, 3, 4, p + 80, q, None) == -1 and "overlap" in err()                      # dx inside g's 96 bytes

    # the max pool's gradient: odd H, odd W, C % 4, misaligned
    assert L.ssd_sn_maxpool_train_backward(p, q, B, 5, 8, 8, q + 8192, None) == -1 and "H" in err() and "even" in err()
    assert L.ssd_sn_maxpool_train_backward(p, q, B, 6, 7, 8, q + 8192, None) == -1 and "even" in err()
    assert L.ssd_sn_maxpool_train_backward(p, q, B, 6, 8, 6, q + 8192, None) == -1 and "C" in err()
    assert L.ssd_sn_maxpool_train_backward(p, q, 0, 6, 8, 8, q + 8192, None) == -1 and "B" in err()
    assert L.ssd_sn_maxpool_train_backward(p, q + 4, B, 6, 8, 8, q + 8192, None) == -1 and "16-byte" in err()
    assert L.ssd_sn_maxpool_train_backward(p, q, B, 6, 8, 8, p, None) == -1 and "alias" in err()
    del keep
