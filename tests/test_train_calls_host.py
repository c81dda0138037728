"""ssd_amd.train_calls, host side (no GPU): the planners through the layer return what the raw symbols return, and the layer's own
checks -- shape, dtype, contiguity, per-channel vectors, level counts, the workspace's dtype, the entry's geometry -- raise
ValueError naming the argument, and correct CPU tensors TypeError, all BEFORE the library is called: ssd_last_error() still holds a
refusal provoked beforehand."""
import contextlib

import pytest
import torch

f32 = torch.float32


@contextlib.contextmanager
def _library_not_called(ssd):
    L = ssd.lib()
    assert L.ssd_depthwise_train_forward(None, 2, 6, 8, 36, None, 3, None, None) == -1      # refused without a GPU: the sentinel
    sentinel = L.ssd_last_error()
    assert sentinel
    yield
    assert L.ssd_last_error() == sentinel


# ----------------------------------------------------------------------------- the planners
def test_planners_through_the_layer_are_the_raw_symbols(ssd):
    L, calls = ssd.lib(), ssd.train_calls
    CL, BL = ssd._lib.SsdConvLevel, ssd._lib.SsdBnLevel
    lv = lambda sizes: (CL * len(sizes))(*[CL(h, w, None, None, None) for h, w in sizes])
    two = [(5, 7), (3, 4)]
    raw = L.ssd_conv3x3_train_workspace_bytes(lv(two), 2, 2, 64, 40)
    assert raw > 0 and calls.conv_workspace_bytes(two, 2, 64, 40, entry="conv3x3") == raw
    assert calls.conv_workspace_bytes(two, 2, 64, 40, 3, 1) == L.ssd_conv_train_workspace_bytes(lv(two), 2, 2, 64, 40, 3, 1, 0) == raw
    assert calls.conv_workspace_bytes([torch.zeros(2, h, w, 64) for h, w in two], 2, 64, 40) == raw     # tensors: only H and W are read
    for k, stride, with_up, sizes in ((1, 1, False, two), (3, 2, False, two), (3, 1, True, [(4, 6)])):
        raw = L.ssd_conv_train_workspace_bytes(lv(sizes), len(sizes), 2, 64, 40, k, stride, int(with_up))
        assert raw > 0 and calls.conv_workspace_bytes(sizes, 2, 64, 40, k, stride, with_up) == raw, (k, stride, with_up)
    raw = L.ssd_pointwise_train_workspace_bytes(lv(two), 2, 2, 64, 40)
    assert raw > 0 and calls.conv_workspace_bytes(two, 2, 64, 40, 1, entry="pointwise") == raw
    rows = [35, 1]
    raw = L.ssd_bn_relu_train_workspace_bytes((BL * 2)(*[BL(r, *([None] * 12)) for r in rows]), 2, 256)
    assert raw > 0 and calls.bn_workspace_bytes(rows, 256) == raw == calls.bn_workspace_bytes([torch.zeros(r, 256) for r in rows], 256)
    raw = L.ssd_depthwise_train_workspace_bytes(2, 6, 8, 36, 2)
    assert raw > 0 and calls.depthwise_workspace_bytes((2, 6, 8, 36), 2) == raw == calls.depthwise_workspace_bytes(torch.zeros(2, 6, 8, 36), 2)
    raw = L.ssd_first_conv_train_workspace_bytes(2, 8, 12, 24)
    assert raw > 0 and calls.first_conv_workspace_bytes((2, 8, 12), 24) == raw
    assert calls.first_conv_workspace_bytes(torch.zeros(2, 8, 12, 3, dtype=torch.uint8), 24) == raw
    with pytest.raises(ValueError, match="conv3x3"):
        calls.conv_workspace_bytes(two, 2, 64, 40, 3, 2, entry="conv3x3")


# ----------------------------------------------------------------------------- correct arguments, on the CPU
def _z(*shape, dtype=f32):
    return torch.zeros(shape, dtype=dtype)


def _good(fn):
    """Correct CPU arguments of ssd_amd.train_calls.<fn>, as keywords: two levels (5,7) and (3,4), B 2, 64 -> 40; depthwise (2,6,8,36)
    at stride 2; first convolution (2,8,12) -> 24; batch norm rows 35 and 1, C 256 (statistics rows padded to 260)."""
    sizes, rows = [(5, 7), (3, 4)], [35, 1]
    xs, ys = [_z(2, h, w, 64) for h, w in sizes], [_z(2, h, w, 40) for h, w in sizes]
    vec = lambda: [_z(260)[:256] for _ in rows]
    bx = [_z(r, 256) for r in rows]
    return {
        "conv_forward": lambda: dict(xs=xs, kernel=_z(3, 3, 64, 40), outs=ys, bias=_z(40)),
        "conv_backward": lambda: dict(xs=xs, kernel=_z(3, 3, 64, 40), dys=ys, dw=_z(3, 3, 64, 40), dxs=[_z(2, h, w, 64) for h, w in sizes], dbias=_z(44)),
        "depthwise_forward": lambda: dict(x=_z(2, 6, 8, 36), kernel=_z(3, 3, 36, 1), out=_z(2, 3, 4, 36), stride=2),
        "depthwise_backward": lambda: dict(x=_z(2, 6, 8, 36), kernel=_z(3, 3, 36, 1), dy=_z(2, 3, 4, 36), dw=_z(3, 3, 36, 1), stride=2, dx=_z(2, 6, 8, 36)),
        "first_conv_forward": lambda: dict(images=_z(2, 8, 12, 3, dtype=torch.uint8), kernel=_z(3, 3, 3, 24), out=_z(2, 4, 6, 24)),
        "first_conv_backward": lambda: dict(images=_z(2, 8, 12, 3, dtype=torch.uint8), dy=_z(2, 4, 6, 24), dw=_z(3, 3, 3, 24)),
        "bn_forward": lambda: dict(xs=bx, outs=[_z(r, 256) for r in rows], gammas=vec(), betas=vec(), training=True, epsilon=1e-3,
                                   one_minus_momentum=0.007, moving_means=vec(), moving_variances=vec(), means=vec(), vars_=vec(), invstds=vec()),
        "bn_backward": lambda: dict(xs=bx, dys=[_z(r, 256) for r in rows], dxs=[_z(r, 256) for r in rows], gammas=vec(), betas=vec(), means=vec(),
                                    invstds=vec(), dgammas=vec(), dbetas=vec()),
    }[fn]()


FUNCTIONS = ["conv_forward", "conv_backward", "depthwise_forward", "depthwise_backward", "first_conv_forward", "first_conv_backward",
             "bn_forward", "bn_backward"]
WITH_WORKSPACE = [f for f in FUNCTIONS if f not in ("depthwise_forward", "first_conv_forward")]


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_correct_cpu_tensors_are_a_type_error(ssd, fn):
    with _library_not_called(ssd):
        with pytest.raises(TypeError, match="no CPU path"):
            getattr(ssd.train_calls, fn)(**_good(fn))


# ----------------------------------------------------------------------------- one defect per call
def _spoil(t, kind):
    if kind == "shape":                                                  # one more row (NHWC) / channel ([rows, C])
        shape = list(t.shape)
        shape[1 if t.dim() == 4 else -1] += 1
        return torch.zeros(shape, dtype=t.dtype)
    if kind == "float64":
        return t.double()
    if kind == "strided":                                                # the right shape, every second element
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]
    assert kind == "short" and t.dim() == 1                              # a per-channel vector one element below C (256 or 40)
    return t[:255 if t.numel() >= 256 else 39].clone()


DEFECTS = [("conv_forward", "outs[1]", "shape"), ("conv_forward", "xs[1]", "float64"), ("conv_forward", "kernel", "strided"), ("conv_forward", "bias", "short"),
           ("conv_backward", "dxs[0]", "shape"), ("conv_backward", "dw", "shape"), ("conv_backward", "dys[1]", "shape"), ("conv_backward", "dys[0]", "float64"),
           ("conv_backward", "dw", "strided"), ("conv_backward", "dbias", "short"),
           ("depthwise_forward", "out", "shape"), ("depthwise_forward", "x", "float64"), ("depthwise_forward", "kernel", "strided"),
           ("depthwise_backward", "dy", "shape"), ("depthwise_backward", "dw", "shape"), ("depthwise_backward", "dx", "shape"),
           ("depthwise_backward", "dy", "float64"), ("depthwise_backward", "dx", "strided"),
           ("first_conv_forward", "out", "shape"), ("first_conv_forward", "images", "float64"), ("first_conv_forward", "kernel", "strided"),
           ("first_conv_backward", "dy", "shape"), ("first_conv_backward", "dw", "shape"), ("first_conv_backward", "dy", "float64"),
           ("first_conv_backward", "dw", "strided"),
           ("bn_forward", "outs[1]", "shape"), ("bn_forward", "xs[0]", "float64"), ("bn_forward", "outs[0]", "strided"), ("bn_forward", "gammas[0]", "short"),
           ("bn_forward", "invstds[1]", "short"), ("bn_forward", "moving_means[0]", "float64"),
           ("bn_backward", "dxs[0]", "shape"), ("bn_backward", "dys[1]", "shape"), ("bn_backward", "dys[0]", "float64"), ("bn_backward", "dxs[1]", "strided"),
           ("bn_backward", "dgammas[0]", "short")]


@pytest.mark.parametrize("fn,target,kind", DEFECTS)
def test_one_defect_is_a_value_error_that_names_the_argument(ssd, fn, target, kind):
    kw = _good(fn)
    name, _, index = target.partition("[")
    if index:
        kw[name] = list(kw[name])
        kw[name][int(index[:-1])] = _spoil(kw[name][int(index[:-1])], kind)
    else:
        kw[name] = _spoil(kw[name], kind)
    with _library_not_called(ssd):
        with pytest.raises(ValueError) as e:
            getattr(ssd.train_calls, fn)(**kw)
    assert target in str(e.value)


def test_per_channel_vectors_may_be_longer_than_c(ssd):
    """conv_backward's dbias has 44 elements for 40 channels and every batch-norm vector is a 256-element view: both pass the shape
    checks and reach the device check."""
    for fn in ("conv_backward", "bn_forward"):
        with pytest.raises(TypeError, match="no CPU path"):
            getattr(ssd.train_calls, fn)(**_good(fn))


@pytest.mark.parametrize("fn,dxs", [("conv_backward", lambda d: d[:1]), ("conv_backward", lambda d: [d[0], None]), ("bn_backward", lambda d: d[:1])])
def test_dxs_for_one_level_of_two_is_a_value_error(ssd, fn, dxs):
    kw = _good(fn)
    kw["dxs"] = dxs(kw["dxs"])
    with _library_not_called(ssd):
        with pytest.raises(ValueError, match="dxs"):
            getattr(ssd.train_calls, fn)(**kw)


@pytest.mark.parametrize("fn", ["conv_forward", "conv_backward", "bn_forward", "bn_backward"])
def test_nine_levels_and_no_level_are_a_value_error(ssd, fn):
    for n in (9, 0):
        kw = {k: ([v[0]] * n if isinstance(v, list) else v) for k, v in _good(fn).items()}
        with _library_not_called(ssd):
            with pytest.raises(ValueError, match="xs: 1 .. 8 levels"):
                getattr(ssd.train_calls, fn)(**kw)
    kw = {k: ([v[0]] * 8 if isinstance(v, list) else v) for k, v in _good(fn).items()}      # eight pass the checks
    with pytest.raises(TypeError, match="no CPU path"):
        getattr(ssd.train_calls, fn)(**kw)


@pytest.mark.parametrize("fn", WITH_WORKSPACE)
def test_a_workspace_that_is_not_uint8_is_a_value_error(ssd, fn):
    for ws in (torch.zeros(1 << 16), torch.zeros((256, 256), dtype=torch.uint8)):
        with _library_not_called(ssd):
            with pytest.raises(ValueError, match="workspace"):
                getattr(ssd.train_calls, fn)(workspace=ws, **_good(fn))


def test_the_entry_fixes_the_geometry(ssd):
    calls = ssd.train_calls
    with _library_not_called(ssd):
        kw = _good("conv_forward")
        with pytest.raises(ValueError, match="conv3x3"):                # stride 2
            calls.conv_forward(**dict(kw, stride=2, outs=[_z(2, 3, 4, 40), _z(2, 2, 2, 40)]), entry="conv3x3")
        with pytest.raises(ValueError, match="conv3x3"):                # k = 1
            calls.conv_forward(**dict(kw, kernel=_z(1, 1, 64, 40)), entry="conv3x3")
        with pytest.raises(ValueError, match="conv3x3"):                # ups
            calls.conv_forward(**dict(kw, bias=None, ups=[_z(2, 2, 3, 40), _z(2, 1, 2, 40)]), entry="conv3x3")
        with pytest.raises(ValueError, match="entry"):                  # the pointwise family has no forward
            calls.conv_forward(**dict(kw, kernel=_z(1, 1, 64, 40)), entry="pointwise")
        kw = _good("conv_backward")
        with pytest.raises(ValueError, match="pointwise"):              # k = 3
            calls.conv_backward(**dict(kw, dbias=None), entry="pointwise")
        with pytest.raises(ValueError, match="pointwise"):              # a dbias
            calls.conv_backward(**dict(kw, kernel=_z(1, 1, 64, 40), dw=_z(1, 1, 64, 40)), entry="pointwise")
        for fn in ("bn_forward", "bn_backward"):
            with pytest.raises(ValueError, match="entry"):              # the old pair is ReLU only
                getattr(calls, fn)(**_good(fn), act="relu6", entry="bn_relu")
            with pytest.raises(ValueError, match="act"):
                getattr(calls, fn)(**_good(fn), act="tanh")
    # and the geometry the arguments imply: stride 2 halves the outputs, ups are half the level
    with pytest.raises(TypeError, match="no CPU path"):
        calls.conv_forward(**dict(_good("conv_forward"), stride=2, outs=[_z(2, 3, 4, 40), _z(2, 2, 2, 40)]))
    with pytest.raises(ValueError, match=r"ups\[1\]"):
        calls.conv_forward(**dict(_good("conv_forward"), bias=None, ups=[_z(2, 2, 3, 40), _z(2, 2, 2, 40)]))
