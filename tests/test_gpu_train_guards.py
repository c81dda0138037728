"""The TRAIN layer kernels, the loss family and ssd_augment's output between guard words at addresses that are 16-byte (or 4-byte)
aligned and no more (include/ssd_hip.h's alignment contract; tests/helpers/guarded.py).  Per case: the call on fresh allocations
(the control, whose values the families' own tests pin), then in one arena per layout; check() finds a store outside a tensor or
into an input, and every output must have the control's bits.  The convolutions run on small integers and are compared exactly
with the float64 restatement as well, so a wrong tail fails even where both runs agree.  Last: contiguous batch slices through the
public ops, the way such addresses arise in practice.  tests/test_guarded_host.py proves that check() can fail."""
import ctypes

import numpy as np
import pytest

from helpers import head_train_ref as href
from helpers import train_ops_ref as tref
from helpers.guarded import LAYOUTS, Arena, Separate

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 2
S2_WIDTHS = [(256, 256), (40, 24)]                                    # tests/test_gpu_fpn_train.py
PAD = f32(-7.5)                                                       # what the pad elements of a padded statistics row hold
_CONTROL, _REFS = {}, {}


def _ints(rng, shape, lo=-3, hi=4):
    return rng.integers(lo, hi, shape).astype(f32)


def _normal(rng, shape, scale=1.0, mean=0.0):
    return rng.normal(mean, scale, shape).astype(f32)


def _assert_bits(name, got, want):
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert g.dtype == w.dtype and g.shape == w.shape, name
    bad = np.nonzero(g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1))[0] if len(g) else []
    assert not len(bad), "'%s': %d of %d elements differ from the control's bits, first at %d: %r against %r" % (
        name, len(np.unique(bad)), len(g), bad[0], g[bad[0]], w[bad[0]])


def _run(cuda, key, layout, case, spares=0):
    """case(memory) adds the call's tensors and makes the call.  Once per key on fresh allocations, then in an arena of `layout`
    (`spares` 4-byte tensors first: they move the contract-4 tensors one residue on) -> the arena's outputs {name: numpy}."""
    if key not in _CONTROL:
        m = Separate(cuda, "cuda")
        case(m)
        cuda.cuda.synchronize()
        m.check()
        _CONTROL[key] = m.outputs()
    a = Arena(cuda, "cuda", layout)
    for i in range(spares):
        a.add("spare%d" % i, (1,), f32, 4, "output")
    case(a)
    cuda.cuda.synchronize()
    a.check()
    got, want = a.outputs(), _CONTROL[key]
    assert set(want) <= set(got) and want
    for name in want:
        _assert_bits(name, got[name], want[name])
    return got


def _views(m, names):
    return None if names is None else [m.view(n) for n in names]


# ----------------------------------------------------------------------------- the convolutions
def _conv_case(ssd, entry, xs, w, stride, mode, bias=None, ups=None, dys=None):
    """mode 'fwd' or 'bwd' with '+bias', '+up', '+dx', '+dbias': the optional pointers that are present.  dbias is exactly Cout
    floats: the guard starts behind element Cout - 1."""
    calls = ssd.train_calls
    k, _, Cin, Cout = w.shape
    opts = set(mode.split("+")[1:])

    def case(m):
        X = [m.add("x%d" % i, x, f32, 16, "input") for i, x in enumerate(xs)]
        m.add("w", w, f32, 16, "input")
        need = calls.conv_workspace_bytes([x.shape[1:3] for x in xs], xs[0].shape[0], Cin, Cout, k, stride, "up" in opts, entry)
        assert need > 0
        m.add("ws", (need,), np.uint8, 16, "workspace")
        if mode.startswith("fwd"):
            b = m.add("bias", bias, f32, 4, "input") if "bias" in opts else None
            U = [m.add("up%d" % i, u, f32, 16, "input") for i, u in enumerate(ups)] if "up" in opts else None
            Y = [m.add("y%d" % i, calls.conv_out_shape(x.shape, Cout, stride), f32, 16, "output") for i, x in enumerate(xs)]
            calls.conv_forward(_views(m, X), m.view("w"), _views(m, Y), stride, m.view(b), _views(m, U), workspace=m.view("ws"), entry=entry)
        else:
            DY = [m.add("dy%d" % i, d, f32, 16, "input") for i, d in enumerate(dys)]
            m.add("dw", w.shape, f32, 16, "output")
            DX = [m.add("dx%d" % i, x.shape, f32, 16, "output") for i, x in enumerate(xs)] if "dx" in opts else None
            db = m.add("dbias", (Cout,), f32, 4, "output") if "dbias" in opts else None
            calls.conv_backward(_views(m, X), m.view("w"), _views(m, DY), m.view("dw"), stride, _views(m, DX), m.view(db),
                                workspace=m.view("ws"), entry=entry)
    return case


def _conv_data(name, sizes, Cin, Cout, k, stride, up, batch=B):
    """Small integers (|x|, |dy|, |up| <= 3, |w| <= 2, |bias| <= 4) and the float64 results, once per case."""
    if name not in _REFS:
        import zlib
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        xs = [_ints(rng, (batch, h, ww, Cin)) for h, ww in sizes]
        dys = [_ints(rng, (batch,) + tref.out_hw(h, ww, stride) + (Cout,)) for h, ww in sizes]
        w, bias = _ints(rng, (k, k, Cin, Cout), -2, 3), _ints(rng, (Cout,), -4, 5)
        ups = [_ints(rng, (batch, h // 2, ww // 2, Cout)) for h, ww in sizes] if up else None
        dw64, db64, dw_abs, db_abs = tref.integer_premise(xs, w, dys, stride)
        assert max(dw_abs, db_abs, 3 * 2 * k * k * max(Cin, Cout) + 7) < 2 ** 24      # every partial sum is exact in float32
        dxs64 = tref.conv_grads(xs, w, dys, stride)[0]
        assert np.abs(dw64).max() > 0
        fwd = {opt: [tref.conv(x, w, stride, u if opt == "up" else None, bias if opt == "bias" else None)
                     for x, u in zip(xs, ups or [None] * len(xs))] for opt in ("", "bias") + (("up",) if up else ())}
        _REFS[name] = dict(xs=xs, dys=dys, w=w, bias=bias, ups=ups, dw=dw64, dbias=db64, dxs=dxs64, fwd=fwd)
    return _REFS[name]


def _conv_check(ssd, cuda, name, entry, sizes, Cin, Cout, k, stride, mode, layout, batch=B):
    d = _conv_data(name, sizes, Cin, Cout, k, stride, " up " in name, batch)
    got = _run(cuda, (name, entry, mode), layout, _conv_case(ssd, entry, d["xs"], d["w"], stride, mode, d["bias"], d["ups"], d["dys"]))
    exact = lambda a, r: a.shape == r.shape and np.array_equal(a.astype(np.float64), r)
    if mode.startswith("fwd"):
        for i, want in enumerate(d["fwd"][mode[4:]]):
            assert exact(got["y%d" % i], want), (name, mode, i)
    else:
        assert exact(got["dw"], d["dw"]), (name, mode)
        if "dx" in mode:
            for i, want in enumerate(d["dxs"]):
                assert exact(got["dx%d" % i], want), (name, mode, i)
        if "dbias" in mode:
            assert exact(got["dbias"], d["dbias"]), (name, mode)


CONV3X3 = ["72-33", "8-1", "256-6", "six-rows", "thin", "eight-levels"]            # head_train_ref.CONV_CASES


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["fwd", "fwd+bias", "bwd", "bwd+dx", "bwd+dbias", "bwd+dx+dbias"])
@pytest.mark.parametrize("name", CONV3X3)
def test_conv3x3(ssd, cuda, name, mode, layout):
    """ssd_conv3x3_train_forward / _backward: Cout = 33, 1 and 6 (a level of [2,1,1,33] is 264 bytes), six rows, thin levels, eight
    levels; with and without bias / dbias, with and without dx."""
    batch, sizes, Cin, Cout = href.CONV_CASES[name]
    _conv_check(ssd, cuda, "3x3 " + name, "conv3x3", sizes, Cin, Cout, 3, 1, mode, layout, batch)


# name: (level sizes, Cin, Cout, k, stride, modes)
CONV = {
    "1x1 116-256": ([(5, 7), (1, 1)], 116, 256, 1, 1, ["fwd", "fwd+bias", "bwd", "bwd+dbias"]),
    "1x1 1024-24": ([(5, 7), (1, 1)], 1024, 24, 1, 1, ["fwd", "fwd+bias", "bwd", "bwd+dbias"]),
    "s2 256-256": ([(5, 7), (1, 1)], 256, 256, 3, 2, ["fwd", "fwd+bias", "bwd", "bwd+dx+dbias"]),
    "s2 40-24": ([(5, 7), (1, 1)], 40, 24, 3, 2, ["fwd", "fwd+bias", "bwd", "bwd+dx+dbias"]),
    "1x1 up 116-256": ([(4, 6), (2, 2)], 116, 256, 1, 1, ["fwd", "fwd+up"]),
    "3x3 up 8-24": ([(4, 6), (2, 2)], 8, 24, 3, 1, ["fwd+up", "bwd+dx"]),
}
assert [(CONV["s2 256-256"][1:3]), (CONV["s2 40-24"][1:3])] == S2_WIDTHS


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,mode", [(n, m) for n, c in CONV.items() for m in c[5]], ids=lambda v: v.replace(" ", "_"))
def test_conv(ssd, cuda, name, mode, layout):
    """ssd_conv_train_forward / _backward: 1x1, 3x3 stride 2 on 5 x 7 and 1 x 1 inputs, `up` on even sizes; two levels each."""
    sizes, Cin, Cout, k, stride, _ = CONV[name]
    _conv_check(ssd, cuda, name, "conv", sizes, Cin, Cout, k, stride, mode, layout)


POINTWISE = [("pointwise", 8, 256, ["bwd", "bwd+dx"]), ("pointwise", 116, 256, ["bwd", "bwd+dx"])] + \
            [("sn_pointwise", ci, co, ["fwd", "bwd", "bwd+dx"]) for ci, co in ((6, 10), (58, 58), (24, 58))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("entry,Cin,Cout,mode", [(e, ci, co, m) for e, ci, co, ms in POINTWISE for m in ms])
def test_pointwise(ssd, cuda, entry, Cin, Cout, mode, layout):
    """ssd_pointwise_train_backward, ssd_sn_pointwise_train_forward / _backward: one level of 5 x 7 and one of 1 x 1, B = 2."""
    _conv_check(ssd, cuda, "%s %d-%d" % (entry, Cin, Cout), entry, [(5, 7), (1, 1)], Cin, Cout, 1, 1, mode, layout)


# ----------------------------------------------------------------------------- the top-down merge
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("optional", ["", "base", "gate", "base+gate"])
@pytest.mark.parametrize("same", [False, True], ids=["upsampled", "same_size"])
@pytest.mark.parametrize("hw", [(2, 2), (6, 10)])
@pytest.mark.parametrize("C", [6, 256])
def test_fpn_merge_backward(ssd, cuda, C, hw, same, optional, layout):
    H, W = hw
    rng = np.random.default_rng(C + H)
    g = _normal(rng, (B, H, W, C) if same else (B, 2 * H, 2 * W, C))
    base, gate = _normal(rng, (B, H, W, C)), _normal(rng, (B, H, W, C))

    def case(m):
        m.add("g", g, f32, 16, "input")
        b = m.add("base", base, f32, 16, "input") if "base" in optional else None
        t = m.add("gate", gate, f32, 16, "input") if "gate" in optional else None
        m.add("out", (B, H, W, C), f32, 16, "output")
        ssd.train_calls.fpn_merge_backward(m.view("g"), m.view(b), m.view(t), same, m.view("out"))
    got = _run(cuda, ("merge", C, hw, same, optional), layout, case)
    assert np.isfinite(got["out"]).all() and np.abs(got["out"]).max() > 0


# ----------------------------------------------------------------------------- the depthwise convolution
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["fwd", "bwd", "bwd+dx"])
@pytest.mark.parametrize("hw", [(5, 7), (2, 2)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("entry,C", [("depthwise", 4), ("depthwise", 36), ("sn_depthwise", 6), ("sn_depthwise", 58)])
def test_depthwise(ssd, cuda, entry, C, stride, hw, mode, layout):
    calls = ssd.train_calls
    rng = np.random.default_rng(C * 10 + stride)
    x, k = _normal(rng, (B,) + hw + (C,)), _normal(rng, (3, 3, C, 1), 0.3)
    oshape = calls.conv_out_shape(x.shape, C, stride)
    dy = _normal(rng, oshape)

    def case(m):
        m.add("x", x, f32, 16, "input")
        m.add("k", k, f32, 16, "input")
        if mode == "fwd":
            m.add("out", oshape, f32, 16, "output")
            calls.depthwise_forward(m.view("x"), m.view("k"), m.view("out"), stride, entry=entry)
            return
        m.add("dy", dy, f32, 16, "input")
        m.add("dw", k.shape, f32, 16, "output")
        dx = m.add("dx", x.shape, f32, 16, "output") if mode == "bwd+dx" else None
        need = calls.depthwise_workspace_bytes(x.shape, stride, entry=entry)
        assert need > 0
        m.add("ws", (need,), np.uint8, 16, "workspace")
        calls.depthwise_backward(m.view("x"), m.view("k"), m.view("dy"), m.view("dw"), stride, m.view(dx), workspace=m.view("ws"), entry=entry)
    got = _run(cuda, ("dw", entry, C, stride, hw, mode), layout, case)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in got.values())


# ----------------------------------------------------------------------------- the batch norm
ROWS = [[1], [9], [1030], [9, 1030]]
BN = [("bn_act", "relu6", C, r) for C in (6, 20, 58, 100) for r in ROWS] + \
     [("sn_bn", "none", C, r) for C in (6, 20, 58, 100) for r in ROWS] + \
     [("bn_relu", "relu", C, [9, 1030]) for C in (6, 20, 58, 100)] + [("bn_act", "relu", C, [9]) for C in (20, 58)]


def _rows_table(n_rows, C, values=None):
    """[n_rows, Cp] float32: a table of per-channel rows packed at exactly C floats where C % 4 == 0 (each row is then 16-byte
    aligned); otherwise rows padded to a multiple of 4 with PAD in the pad elements.  NaN where no values are given."""
    Cp = (C + 3) // 4 * 4
    t = np.full((n_rows, Cp), np.nan, f32)
    if values is not None:
        t[:, :C] = values
    t[:, C:] = PAD
    return t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["train", "train-bare", "infer", "bwd"])
@pytest.mark.parametrize("entry,act,C,rows", BN, ids=["%s-%s-%d-%s" % (e, a, C, "x".join(map(str, r))) for e, a, C, r in BN])
def test_batch_norm(ssd, cuda, entry, act, C, rows, mode, layout):
    """ssd_bn_relu_train_*, ssd_bn_act_train_* (relu, relu6), ssd_sn_bn_train_* (none).  train: every pointer present; train-bare:
    no moving statistics, no var; infer: the moving statistics are inputs, nothing else is written, the workspace is NULL; bwd.
    Per level the parameters, the moving statistics, the batch statistics and the two gradients are tables of rows (_rows_table);
    a pad element must keep PAD."""
    calls = ssd.train_calls
    rng = np.random.default_rng(C * 7 + len(rows))
    n = len(rows)
    xs = [_normal(rng, (r, C), 2.0, 1.0) for r in rows]
    dys = [_normal(rng, (r, C)) for r in rows]
    affine = [_rows_table(2, C, np.stack([rng.uniform(0.5, 1.5, C), rng.normal(0, 0.5, C)])) for _ in rows]
    moving = [_rows_table(2, C, np.stack([rng.normal(0, 1, C), rng.uniform(0.5, 2.0, C)])) for _ in rows]
    saved = [_rows_table(2, C, np.stack([x.mean(0), href.invstd_f32(x.var(0))])) for x in xs]      # any statistics serve the backward
    eps, omm = float(f32(href.EPS)), float(f32(1.0 - href.MOMENTUM))
    how = dict(entry=entry, act=act)

    def case(m):
        X = [m.add("x%d" % i, x, f32, 16, "input") for i, x in enumerate(xs)]
        A = [m.add("affine%d" % i, a, f32, 16, "input") for i, a in enumerate(affine)]
        col = lambda names, j: None if names is None else [m.view(t)[j, :C] for t in names]
        if mode == "bwd":
            DY = [m.add("dy%d" % i, d, f32, 16, "input") for i, d in enumerate(dys)]
            S = [m.add("saved%d" % i, s, f32, 16, "input") for i, s in enumerate(saved)]
            DX = [m.add("dx%d" % i, x.shape, f32, 16, "output") for i, x in enumerate(xs)]
            G = [m.add("grads%d" % i, (2, affine[0].shape[1]), f32, 16, "output", fill=_rows_table(2, C)) for i in range(n)]
            m.add("ws", (calls.bn_workspace_bytes(rows, C),), np.uint8, 16, "workspace")
            calls.bn_backward(_views(m, X), _views(m, DY), _views(m, DX), col(A, 0), col(A, 1), col(S, 0), col(S, 1), col(G, 0), col(G, 1),
                              workspace=m.view("ws"), **how)
            return
        Y = [m.add("y%d" % i, x.shape, f32, 16, "output") for i, x in enumerate(xs)]
        if mode == "infer":
            M = [m.add("moving%d" % i, v, f32, 16, "input") for i, v in enumerate(moving)]
            calls.bn_forward(_views(m, X), _views(m, Y), col(A, 0), col(A, 1), False, eps, 0.0, col(M, 0), col(M, 1),
                             workspace=m.torch.empty(0, dtype=m.torch.uint8, device="cuda"), **how)
            return
        M = [m.add("moving%d" % i, v.shape, f32, 16, "output", fill=v) for i, v in enumerate(moving)] if mode == "train" else None
        S = [m.add("stats%d" % i, (3, affine[0].shape[1]), f32, 16, "output", fill=_rows_table(3, C)) for i in range(n)]
        m.add("ws", (calls.bn_workspace_bytes(rows, C),), np.uint8, 16, "workspace")
        calls.bn_forward(_views(m, X), _views(m, Y), col(A, 0), col(A, 1), True, eps, omm, col(M, 0), col(M, 1), col(S, 0),
                         col(S, 1) if mode == "train" else None, col(S, 2), workspace=m.view("ws"), **how)
    got = _run(cuda, ("bn", entry, act, C, tuple(rows), mode), layout, case)
    for name, v in got.items():
        if v.ndim == 2 and v.shape[0] in (2, 3) and name[:-1] in ("moving", "stats", "grads"):
            assert (v[:, C:] == PAD).all(), name                                   # the pad elements of a padded row
            written = v[[0, 2] if (name.startswith("stats") and mode == "train-bare") else slice(None), :C]
            assert np.isfinite(written).all(), name
        else:
            assert np.isfinite(v).all(), name
    if mode == "train":
        assert all(not np.array_equal(got["moving%d" % i], moving[i]) for i in range(n))


# ----------------------------------------------------------------------------- the first convolution
@pytest.mark.parametrize("layout", ["aligned", "skewed-4", "skewed-8", "skewed-12", "mixed", "skewed-f32", "mixed-f32", "aligned-f32"])
@pytest.mark.parametrize("mode", ["fwd", "bwd"])
@pytest.mark.parametrize("batch,hw", [(1, (6, 10)), (3, (6, 10)), (1, (32, 32)), (3, (32, 32))])
@pytest.mark.parametrize("Cout", [8, 24, 32])
def test_first_conv(ssd, cuda, Cout, batch, hw, mode, layout):
    """ssd_first_conv_train_* on uint8 frames (contract 4: byte residues 4, 8 and 12 past a 16-byte boundary) and
    ssd_first_conv_f32_train_* on float frames (layouts *-f32, contract 16)."""
    calls = ssd.train_calls
    f32_frames = layout.endswith("-f32")
    kind, _, tail = layout.partition("-")
    spares = 0 if f32_frames or not tail else int(tail) // 4 - 1
    rng = np.random.default_rng(Cout + batch + hw[0])
    frames = rng.integers(0, 256, (batch,) + hw + (3,), dtype=np.uint8)
    images = rng.uniform(0, 1, frames.shape).astype(f32) if f32_frames else frames
    k, dy = _normal(rng, (3, 3, 3, Cout), 0.3), _normal(rng, (batch, hw[0] // 2, hw[1] // 2, Cout))
    fwd, bwd, need = ((calls.first_conv_f32_forward, calls.first_conv_f32_backward, calls.first_conv_f32_workspace_bytes) if f32_frames
                      else (calls.first_conv_forward, calls.first_conv_backward, calls.first_conv_workspace_bytes))

    def case(m):
        m.add("images", images, images.dtype, 16 if f32_frames else 4, "input")
        if mode == "fwd":
            m.add("k", k, f32, 16, "input")
            m.add("out", dy.shape, f32, 16, "output")
            fwd(m.view("images"), m.view("k"), m.view("out"))
            return
        m.add("dy", dy, f32, 16, "input")
        m.add("dw", k.shape, f32, 16, "output")
        nbytes = need(images.shape, Cout)
        assert nbytes > 0
        m.add("ws", (nbytes,), np.uint8, 16, "workspace")
        bwd(m.view("images"), m.view("dy"), m.view("dw"), workspace=m.view("ws"))
    got = _run(cuda, ("first", f32_frames, Cout, batch, hw, mode), kind, case, spares)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for n, v in got.items() if not n.startswith("spare"))


# ----------------------------------------------------------------------------- ShuffleNet's copies and its max pool
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("D", [1, 2, 58])
@pytest.mark.parametrize("op", ["shuffle", "shuffle-transpose", "concat", "split"])
def test_shufflenet_copies(ssd, cuda, op, D, rows, layout):
    """ssd_sn_shuffle_train (both directions), ssd_sn_concat_train, ssd_sn_split_train: element-wise, 8-byte and (D = 58: 232-byte
    rows) mixed accesses; every word is a distinct bit pattern, so a misplaced copy shows."""
    calls = ssd.train_calls
    words = np.arange(1, 4 * rows * D + 1, dtype=np.uint32) * np.uint32(2654435761)
    a, b, wide = words[:rows * D].view(f32).reshape(rows, D), words[rows * D:2 * rows * D].view(f32).reshape(rows, D), \
        words[2 * rows * D:].view(f32).reshape(rows, 2 * D)

    def case(m):
        if op == "split":
            m.add("g", wide, f32, 16, "input")
            m.add("dx", (rows, D), f32, 16, "output")
            m.add("dy", (rows, D), f32, 16, "output")
            calls.split(m.view("g"), m.view("dx"), m.view("dy"))
            return
        m.add("x", a, f32, 16, "input")
        m.add("y", b, f32, 16, "input")
        if op == "concat":
            m.add("out", (rows, 2 * D), f32, 16, "output")
            calls.concat(m.view("x"), m.view("y"), m.view("out"))
        else:
            m.add("xo", (rows, D), f32, 16, "output")
            m.add("yo", (rows, D), f32, 16, "output")
            calls.shuffle(m.view("x"), m.view("y"), m.view("xo"), m.view("yo"), transpose=op == "shuffle-transpose")
    got = _run(cuda, ("copy", op, D, rows), layout, case)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)
    if op == "split":
        want = {"dx": wide[:, :D], "dy": wide[:, D:]}
    elif op == "concat":
        want = {"out": np.concatenate([a, b], 1)}
    elif op == "shuffle":
        z = np.stack([bits(a), bits(b)], 2).reshape(rows, 2 * D).view(f32)
        want = {"xo": z[:, :D], "yo": z[:, D:]}
    else:
        dz = np.concatenate([bits(a), bits(b)], 1).view(f32)
        want = {"xo": dz[:, 0::2], "yo": dz[:, 1::2]}
    for name, w in want.items():
        assert np.array_equal(bits(got[name]), bits(w)), name


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(4, 6), (8, 8)])
@pytest.mark.parametrize("C", [8, 24])
def test_maxpool_backward(ssd, cuda, C, hw, layout):
    rng = np.random.default_rng(C + hw[0])
    x = _ints(rng, (B,) + hw + (C,))                                     # ties everywhere: the winner rule decides
    dy = _normal(rng, (B, hw[0] // 2, hw[1] // 2, C))

    def case(m):
        m.add("x", x, f32, 16, "input")
        m.add("dy", dy, f32, 16, "input")
        m.add("dx", x.shape, f32, 16, "output")
        ssd.train_calls.maxpool_backward(m.view("x"), m.view("dy"), m.view("dx"))
    got = _run(cuda, ("pool", C, hw), layout, case)
    assert np.isfinite(got["dx"]).all() and np.abs(got["dx"]).max() > 0


# ----------------------------------------------------------------------------- the loss family
GAMMA, ALPHA = 2.0, 0.25
RESIDUE = {1: 0, 3: 1, 80: 2}          # spare 4-byte tensors in front, per C: skewed logits land 4, 8 and 12 bytes past a 16-byte boundary


def _loss_inputs(ssd, cuda, C, G):
    """128 x 128 anchors, B = 2: logits, codes, ground truth around random anchors (a duplicate box), and -- from the public wrappers on
    fresh allocations -- the targets and per_image rows that ssd_loss_backward reads."""
    key = ("loss inputs", C, G)
    if key not in _REFS:
        gen = ssd.AnchorGenerator()
        anchors = np.ascontiguousarray(gen(128, 128), dtype=f32)
        levels = tuple(int(v) for v in gen.num_anchors_per_feature_map)
        N = len(anchors)
        rng = np.random.default_rng(C * 100 + G)
        counts = [G, max(G // 3, 1)]
        boxes = np.zeros((B, G, 4), f32)
        for b, cnt in enumerate(counts):
            a = anchors[rng.integers(0, N, cnt)].astype(np.float64)
            boxes[b, :cnt] = a + rng.normal(0, 0.05, (cnt, 4)) * (a[:, 2:3] - a[:, 0:1])
            if cnt >= 2:
                boxes[b, 1] = boxes[b, 0]
        labels, num = rng.integers(0, C, (B, G)).astype(np.int32), np.array(counts, np.int32)
        logits, codes = _normal(rng, (B, N, C), 3.0, -3.0), _normal(rng, (B, N, 4), 1.5)
        dev = lambda v: cuda.from_numpy(v).cuda()
        reg, cls, matches = ssd.get_training_targets(dev(anchors), boxes, labels, num)
        _, per = ssd.ssd_loss(dev(logits), dev(codes), dev(anchors), {"boxes": boxes, "labels": labels, "num_boxes": num},
                              gamma=GAMMA, alpha=ALPHA, anchors_per_level=levels)
        assert int((matches >= 0).sum()) > 0
        _REFS[key] = dict(anchors=anchors, levels=levels, N=N, boxes=boxes, labels=labels, num=num, logits=logits, codes=codes,
                          reg=reg.cpu().numpy(), cls=cls.cpu().numpy(), matches=matches.cpu().numpy(), per=per.cpu().numpy())
    return _REFS[key]


def _raw(ssd, cuda, m, fn, *args):
    """A raw ctypes call of the library: names of the memory's tensors become their addresses, None NULL."""
    L = ssd.lib()
    a = [ctypes.c_void_p(m.ptr(v[1])) if isinstance(v, tuple) else v for v in args]
    rc = getattr(L, fn)(*a, ctypes.c_void_p(cuda.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ssd_last_error()


def _groundtruth(m, d):
    m.add("anchors", d["anchors"], f32, 16, "input")
    m.add("boxes", d["boxes"], f32, 16, "input")
    m.add("labels", d["labels"], np.int32, 4, "input")
    m.add("num", d["num"], np.int32, 4, "input")


P = lambda name: ("ptr", name)                                         # _raw: the address of this tensor of the memory


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("outputs", ["all", "matches-only"])
@pytest.mark.parametrize("G", [1, 17])
def test_training_targets(ssd, cuda, G, outputs, layout):
    d = _loss_inputs(ssd, cuda, 3, G)
    N = d["N"]
    cfg = ssd.ssd._loss_config(0.5, 0.5)

    def case(m):
        _groundtruth(m, d)
        reg = m.add("reg", (B, N, 4), f32, 16, "output") if outputs == "all" else None
        cls = m.add("cls", (B, N), np.int32, 4, "output") if outputs == "all" else None
        m.add("matches", (B, N), np.int32, 4, "output")
        need = ssd.lib().ssd_loss_workspace_bytes(B, N, G)
        m.add("ws", (need,), np.uint8, 16, "workspace")
        _raw(ssd, cuda, m, "ssd_training_targets", P("anchors"), N, P("boxes"), P("labels"), P("num"), B, G, ctypes.byref(cfg),
             P(reg), P(cls), P("matches"), P("ws"), need)
    got = _run(cuda, ("targets", G, outputs), layout, case)
    assert np.array_equal(got["matches"], d["matches"])
    if outputs == "all":
        assert np.array_equal(got["cls"], d["cls"]) and np.array_equal(got["reg"].view(np.uint32), d["reg"].view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("outputs", ["all", "losses-only"])
@pytest.mark.parametrize("G", [1, 17])
@pytest.mark.parametrize("C", [1, 3, 80])
def test_loss(ssd, cuda, C, G, outputs, layout):
    """ssd_loss: logits at the 4-byte residues, codes, anchors and boxes skewed, every optional output present or NULL."""
    d = _loss_inputs(ssd, cuda, C, G)
    N, levels = d["N"], d["levels"]
    cfg = ssd.ssd._loss_config(0.5, 0.5, GAMMA, ALPHA, levels)

    def case(m):
        m.add("logits", d["logits"], f32, 4, "input")
        m.add("codes", d["codes"], f32, 16, "input")
        _groundtruth(m, d)
        m.add("losses", (2,), f32, 4, "output")
        every = outputs == "all"
        per = m.add("per_image", (B, 3 + len(levels)), f32, 4, "output") if every else None
        cl = m.add("cls_losses", (B, N), f32, 4, "output") if every else None
        ll = m.add("loc_losses", (B, N), f32, 4, "output") if every else None
        need = ssd.lib().ssd_loss_workspace_bytes(B, N, G)
        m.add("ws", (need,), np.uint8, 16, "workspace")
        _raw(ssd, cuda, m, "ssd_loss", P("logits"), P("codes"), P("anchors"), B, N, C, P("boxes"), P("labels"), P("num"), G,
             ctypes.byref(cfg), P(per), P("losses"), P(cl), P(ll), P("ws"), need)
    got = _run(cuda, ("loss", C, G, outputs), layout, case, spares=RESIDUE[C])
    assert np.isfinite(got["losses"]).all() and got["losses"].min() > 0
    if outputs == "all":
        assert np.array_equal(got["per_image"].view(np.uint32), d["per"].view(np.uint32))
        assert np.isfinite(got["cls_losses"]).all() and np.isfinite(got["loc_losses"]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("upstream", [True, False], ids=["grad_losses", "null"])
@pytest.mark.parametrize("G", [1, 17])
@pytest.mark.parametrize("C", [1, 3, 80])
def test_loss_backward(ssd, cuda, C, G, upstream, layout):
    """ssd_loss_backward: logits and d_logits at the 4-byte residues, codes, reg_targets and d_codes skewed."""
    d = _loss_inputs(ssd, cuda, C, G)
    N = d["N"]
    cfg = ssd.ssd._loss_config(0.5, 0.5, GAMMA, ALPHA)

    def case(m):
        m.add("logits", d["logits"], f32, 4, "input")
        m.add("codes", d["codes"], f32, 16, "input")
        m.add("reg", d["reg"], f32, 16, "input")
        m.add("cls", d["cls"], np.int32, 4, "input")
        m.add("matches", d["matches"], np.int32, 4, "input")
        m.add("per_image", d["per"], f32, 4, "input")
        g = m.add("grad_losses", np.array([1.5, -2.0], f32), f32, 4, "input") if upstream else None
        m.add("d_logits", (B, N, C), f32, 4, "output")
        m.add("d_codes", (B, N, 4), f32, 16, "output")
        _raw(ssd, cuda, m, "ssd_loss_backward", P("logits"), P("codes"), B, N, C, P("reg"), P("cls"), P("matches"), P("per_image"),
             d["per"].shape[1], ctypes.byref(cfg), P(g), P("d_logits"), P("d_codes"))
    got = _run(cuda, ("loss backward", C, G, upstream), layout, case, spares=RESIDUE[C])
    assert np.isfinite(got["d_logits"]).all() and np.count_nonzero(got["d_logits"]) and np.count_nonzero(got["d_codes"])


# ----------------------------------------------------------------------------- the augmentation's output
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("channels_first", [False, True], ids=["nhwc", "nchw"])
def test_augment_output(ssd, cuda, channels_first, layout):
    """ssd_augment: `out` alone in the arena (the frames are gathered as bytes at any offset, which the augment tests cover), B = 3,
    128 x 128, both output formats; the control is compared with the float32 restatement once."""
    from helpers import augment_ref
    from ssd_amd import augment
    rng = np.random.default_rng(31)
    shapes, flags, hw = [(33, 17), (7, 5), (127, 129)], [15, 0, 12], (128, 128)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    p = np.zeros(3, augment.PARAMS_DTYPE)
    at = 0
    for b, ((H, W), fl) in enumerate(zip(shapes, flags)):
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        p[b]["offset"], p[b]["height"], p[b]["width"], p[b]["flags"] = at, H, W, fl
        p[b]["crop_y"], p[b]["crop_x"], p[b]["crop_h"], p[b]["crop_w"] = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
        p[b]["color_offset"] = augment.color_offsets(rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
        p[b]["scale_min"], p[b]["scale_range"] = f32(0.85), f32(1.15) - f32(0.85)
        p[b]["philox_key"] = rng.integers(0, 2 ** 64, dtype=np.uint64)
        at += frames[b].size
    images = cuda.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    rows = cuda.from_numpy(p.view(np.uint8).copy()).cuda()
    shape = (3, 3) + hw if channels_first else (3,) + hw + (3,)

    def case(m):
        m.add("out", shape, f32, 16, "output")
        L = ssd.lib()
        rc = L.ssd_augment(images.data_ptr(), p.ctypes.data_as(ctypes.c_void_p), rows.data_ptr(), 3, hw[0], hw[1], int(channels_first),
                           m.ptr("out"), ctypes.c_void_p(cuda.cuda.current_stream().cuda_stream))
        assert rc == 0, L.ssd_last_error()
    got = _run(cuda, ("augment", channels_first), layout, case)
    if ("augment ref", channels_first) not in _REFS:
        _REFS[("augment ref", channels_first)] = np.stack([augment_ref.augment(f, q, hw[0], hw[1], channels_first) for f, q in zip(frames, p)])
    assert np.array_equal(got["out"].view(np.uint32), _REFS[("augment ref", channels_first)].view(np.uint32))


# ----------------------------------------------------------------------------- contiguous views through the public ops
def _slice_check(cuda, op, inputs, params=(), states=(), odd=()):
    """op(inputs, params, states) -> a tensor or a list of them, differentiated once with upstream gradients that are batch slices
    too.  inputs: [(array [4, ...], requires a gradient)]; x[1:3] of each is contiguous and passes .contiguous() unchanged.  The
    outputs, every gradient and the states (updated in place) must have the bits of the same call on x[1:3].clone(), and the four
    images of every batch tensor must be unchanged afterwards.  odd: indices of the inputs whose slice must start at a 16-byte
    address that is no multiple of 32."""
    dev = lambda a: cuda.from_numpy(np.ascontiguousarray(a)).cuda()
    four = [dev(a) for a, _ in inputs]
    runs, grads4 = [], None
    for clone in (False, True):
        ins = []
        for i, (t, (_, needs)) in enumerate(zip(four, inputs)):
            v = t[1:3].clone() if clone else t[1:3].detach()
            assert v.is_contiguous() and (clone or v.data_ptr() == t.data_ptr() + t[0].numel() * t.element_size())
            if i in odd and not clone:
                assert v.data_ptr() % 32 == 16, "input %d: the slice must be 16-byte aligned and not 32" % i
            ins.append(v.requires_grad_() if needs else v)
        ps = [dev(a).requires_grad_() for a in params]
        ss = [dev(a) for a in states]
        outs = op(ins, ps, ss)
        outs = [outs] if isinstance(outs, cuda.Tensor) else list(outs)
        if grads4 is None:
            rng = np.random.default_rng(77)
            grads4 = [dev(_normal(rng, (4,) + tuple(o.shape[1:]))) if o.dim() else None for o in outs]
            grads4_host = [None if g is None else g.cpu().numpy() for g in grads4]
        ups = [cuda.ones_like(o) if g is None else (g[1:3].clone() if clone else g[1:3]) for o, g in zip(outs, grads4)]
        cuda.autograd.backward(outs, ups)
        runs.append([o.detach().cpu().numpy() for o in outs] + [t.grad.cpu().numpy() for t in ins if t.requires_grad]
                    + [q.grad.cpu().numpy() for q in ps] + [s.cpu().numpy() for s in ss])
    assert len(runs[0]) == len(runs[1]) and len(runs[0]) > len(states)
    for i, (a, b) in enumerate(zip(*runs)):
        _assert_bits("result %d" % i, a, b)
        assert np.isfinite(a).all()
    for t, (a, _) in zip(four, inputs):
        _assert_bits("a batch tensor after the call", t.cpu().numpy(), np.ascontiguousarray(a))
    for g, h in zip(grads4, grads4_host):
        if g is not None:
            _assert_bits("an upstream gradient after the call", g.cpu().numpy(), h)


def _bn_op(ssd, act):
    return lambda ins, ps, ss: ssd.batch_norm_act(ins[0], ps[0], ps[1], ss[0], ss[1], True, act=act) if act != "relu" else \
        ssd.batch_norm_relu(ins[0], ps[0], ps[1], ss[0], ss[1], True)


def _public_ops(ssd, rng):
    """name: (op, inputs, params, states, odd).  A slice x[1:] starts one image into the allocation; it is a 16-byte address that
    is no multiple of 32 exactly when an image has 4 (mod 8) floats: 5 x 7 x 36, 5 x 7 x 116, 6 x 5 x 58, 6 x 10 x 3.  (5 x 7 x 58
    floats are 8 (mod 16) bytes: an address the header refuses.)  A 3x3 kernel takes Cin % 8 == 0 and the max pool even sizes with
    C % 4 == 0: their images are multiples of 32 bytes, and only the upstream gradient (Cout = 36; 3 x 3 x 36) is odd there."""
    n, u = lambda *s: _normal(rng, s), lambda *s: rng.uniform(0.5, 1.5, s).astype(f32)
    bn = lambda C: ([u(C), n(C)], [n(C), u(C)])
    return {
        "conv_same": (lambda i, p, s: ssd.conv_same(i[0], p[0]), [(n(4, 5, 7, 116), False)], [n(1, 1, 116, 36)], [], [0]),
        "conv_same-s2": (lambda i, p, s: ssd.conv_same(i[0], p[0], stride=2), [(n(4, 5, 7, 8), True)], [n(3, 3, 8, 36)], [], []),
        "conv3x3_same": (lambda i, p, s: ssd.conv3x3_same(i[0], p[0], p[1]), [(n(4, 5, 7, 8), True)], [n(3, 3, 8, 36), n(36)], [], []),
        "depthwise_conv-36-s2": (lambda i, p, s: ssd.depthwise_conv(i[0], p[0], 2), [(n(4, 5, 7, 36), True)], [n(3, 3, 36, 1)], [], [0]),
        "depthwise_conv-58": (lambda i, p, s: ssd.depthwise_conv(i[0], p[0], 1), [(n(4, 6, 5, 58), True)], [n(3, 3, 58, 1)], [], [0]),
        "pointwise_conv-36": (lambda i, p, s: ssd.pointwise_conv(i[0], p[0]), [(n(4, 5, 7, 36), True)], [n(1, 1, 36, 24)], [], [0]),
        "pointwise_conv-58": (lambda i, p, s: ssd.pointwise_conv(i[0], p[0]), [(n(4, 6, 5, 58), True)], [n(1, 1, 58, 58)], [], [0]),
        "batch_norm_relu": (_bn_op(ssd, "relu"), [(n(4, 5, 7, 36), True)], *bn(36), [0]),
        "batch_norm_act-relu6": (_bn_op(ssd, "relu6"), [(n(4, 6, 5, 58), True)], *bn(58), [0]),
        "batch_norm_act-none": (_bn_op(ssd, "none"), [(n(4, 6, 5, 58), True)], *bn(58), [0]),
        "first_conv_train_float": (lambda i, p, s: ssd.first_conv_train_float(i[0], p[0]),
                                   [(rng.uniform(0, 1, (4, 6, 10, 3)).astype(f32), False)], [n(3, 3, 3, 24)], [], [0]),
        "concat_shuffle_split": (lambda i, p, s: ssd.concat_shuffle_split(i[0], i[1]), [(n(4, 6, 5, 58), True), (n(4, 6, 5, 58), True)],
                                 [], [], [0, 1]),
        "maxpool3x3s2_train": (lambda i, p, s: ssd.maxpool3x3s2_train(i[0]), [(n(4, 6, 6, 36), True)], [], [], []),
    }


PUBLIC = ["conv_same", "conv_same-s2", "conv3x3_same", "depthwise_conv-36-s2", "depthwise_conv-58", "pointwise_conv-36", "pointwise_conv-58",
          "batch_norm_relu", "batch_norm_act-relu6", "batch_norm_act-none", "first_conv_train_float", "concat_shuffle_split",
          "maxpool3x3s2_train"]


@pytest.mark.parametrize("name", PUBLIC)
def test_batch_slices_through_the_public_ops(ssd, cuda, name):
    ops = _public_ops(ssd, np.random.default_rng(PUBLIC.index(name)))
    assert list(ops) == PUBLIC
    _slice_check(cuda, *ops[name])


@pytest.mark.parametrize("C", [3, 80])
def test_batch_slices_through_the_differentiable_loss(ssd, cuda, C):
    """Logits [4,N,C] (C = 3: an image is 8 (mod 16) bytes, the 4-byte contract) and codes [4,N,4] (N is even: 32 (mod 64) bytes)."""
    d = _loss_inputs(ssd, cuda, C, 17)
    rng = np.random.default_rng(C)
    logits4, codes4 = _normal(rng, (4, d["N"], C), 3.0, -3.0), _normal(rng, (4, d["N"], 4), 1.5)
    logits4[1:3], codes4[1:3] = d["logits"], d["codes"]
    anchors = cuda.from_numpy(d["anchors"]).cuda()
    gt = {"boxes": d["boxes"], "labels": d["labels"], "num_boxes": d["num"]}

    def op(ins, ps, ss):
        out = ssd.differentiable_loss(ins[0], ins[1], anchors, gt, {"gamma": GAMMA, "alpha": ALPHA})
        return [out["localization_loss"], out["classification_loss"]]
    _slice_check(cuda, op, [(logits4, True), (codes4, True)])
