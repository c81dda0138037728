"""The TRAIN first convolution from float frames on the GPU (include/ssd_hip.h, the header block of that name): the raw forward against
the CPU oracle's conv2d(q(x), w, 2) bit for bit on full-mantissa frames, the weight gradient exactly on the 2^-12 grid and within the
bound of a double sum rounded once on full-mantissa frames, its determinism, the last row and column, the equivalence with the uint8
block on byte-grid frames bit for bit -- kernels and both trainable backbones, Conv2d_0 / Conv1 trained and frozen, .train() and
.eval() --, and the refusals."""
import numpy as np
import pytest

from helpers import first_conv_f32_ref as ref
from helpers import first_conv_train_ref as uref
from helpers import head_train_ref as href
from helpers.backbone_train_gpu import fc_backward_dev
from helpers.head_train_gpu import dev as _dev, same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
SIZES = [(2, 2), (4, 6), (6, 8), (10, 14), (32, 32)]                  # odd and even output columns; (2,2): one output, ky = 2 and kx = 2 outside
WIDTHS = [4, 8, 24, 32]                                               # 4: the chunk-of-4 kernel; 24: G = 6 does not divide 256
BATCHES = [1, 3]
SN_PARAMS = dict(TINY_PARAMS, backbone="shufflenet")


def _fwd(ssd, cuda, img, k):
    return ref.f32_forward_dev(ssd, cuda, _dev(cuda, img), _dev(cuda, k)).cpu().numpy()


def _dw(ssd, cuda, img, dy, fill_ws=None):
    return ref.f32_backward_dev(ssd, cuda, _dev(cuda, img), _dev(cuda, dy), fill_ws).cpu().numpy()


# ----------------------------------------------------------------------------- 1. the forward
def _forward_case(ssd, cuda, oracle_ops, rng, B, H, W, Cout):
    img = ref.full_mantissa_frames(rng, B, H, W)
    k = rng.normal(0, 0.5, (3, 3, 3, Cout)).astype(f32)
    y = _fwd(ssd, cuda, img, k)                                          # out pre-filled with NaN
    want = oracle_ops.conv2d(ref.q(img), k, stride=2)
    assert y.shape == (B, H // 2, W // 2, Cout) and same_bits(y, want) and np.abs(want).max() > 0, (B, H, W, Cout)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Cout", WIDTHS)
def test_forward_is_the_oracles_convolution_of_q_bit_for_bit(ssd, cuda, oracle_ops, Cout, B):
    """(10,14) with B = 3 is 105 outputs: a full wave and a ragged one; (32,32) with B = 3 three blocks."""
    rng = np.random.default_rng(Cout + B)
    for H, W in SIZES:
        _forward_case(ssd, cuda, oracle_ops, rng, B, H, W, Cout)


def test_forward_at_64_channels(ssd, cuda, oracle_ops):
    """The widest first layer: 68 KB of transpose rows, the opt-in LDS size."""
    _forward_case(ssd, cuda, oracle_ops, np.random.default_rng(64), 3, 10, 14, 64)


def test_forward_takes_values_outside_0_1_as_ieee_arithmetic_does(ssd, cuda, oracle_ops):
    """No clamp: -0.25 -> -1.5, 1.5 -> 2, 3e38 -> inf (2x overflows) on the oracle and on the GPU alike.  The infinity sits at
    [0, 0, 0, 0], which only output (0, 0) reads; the weights are positive there so no inf - inf arises."""
    rng = np.random.default_rng(5)
    B, H, W, Cout = 1, 6, 8, 8
    img = ref.full_mantissa_frames(rng, B, H, W)
    img[0, 2, 3], img[0, 5, 7] = f32(-0.25), f32(1.5)
    img[0, 0, 0, 0] = f32(3e38)
    k = np.abs(rng.normal(0, 0.5, (3, 3, 3, Cout))).astype(f32) + f32(0.01)
    y = _fwd(ssd, cuda, img, k)
    with np.errstate(over="ignore"):
        want = oracle_ops.conv2d(ref.q(img), k, stride=2)
    assert same_bits(y, want) and np.isinf(y[0, 0, 0]).all() and np.isfinite(y[0, 1:]).all()


# ----------------------------------------------------------------------------- 2. the weight gradient
def _exact_case(ssd, cuda, B, H, W, Cout, seed):
    """Frames on the 2^-12 grid: q is a multiple of 2^-11 in [-1, 1]; integer dy in [-8, 8]: every term is a multiple of 2^-11 of
    magnitude at most 8, so a sum of R of them stays below R * 2^14 units of 2^-11 -- far below 2^53 (asserted) --, every double
    addition is exact in any order, and dw must be float32(the float64 sum) on every element."""
    rng = np.random.default_rng(seed)
    img = ref.grid_frames(rng, B, H, W)
    dy = rng.integers(-8, 9, (B, H // 2, W // 2, Cout)).astype(f32)
    terms = ref.fc_terms(img, dy)
    units = terms * 2.0 ** 11
    assert np.array_equal(units, np.round(units)) and np.abs(units).sum(0).max() < 2.0 ** 53
    want = terms.sum(0).reshape(3, 3, 3, Cout)
    dw = _dw(ssd, cuda, img, dy)
    assert dw.shape == want.shape and same_bits(dw, want.astype(f32)), (B, H, W, Cout)
    return want


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Cout", WIDTHS)
def test_weight_gradient_is_exact_on_the_grid(ssd, cuda, Cout, B):
    for H, W in SIZES:
        want = _exact_case(ssd, cuda, B, H, W, Cout, Cout * 100 + B * 10 + H)
        assert np.abs(want).max() > 0
        if (H, W) == (2, 2):
            assert not want[2].any() and not want[:, 2].any()


def test_weight_gradient_is_exact_over_one_two_and_three_slabs(ssd, cuda):
    """32 channels: G = 8, rpp = 32 row lanes, slab_rows = max(8 * 32, ceil(R / 1024)) = 256.  B frames of 32 x 32 are R = 256 B output
    rows: exactly one, two and three full slabs for B = 1, 2, 3; the workspace is [slabs][27][32] doubles."""
    for B in (1, 2, 3):
        assert uref.slab_plan(256 * B, 32) == (32, 256, B)
        assert ssd.train_calls.first_conv_f32_workspace_bytes((B, 32, 32), 32) == B * 27 * 32 * 8
        assert np.abs(_exact_case(ssd, cuda, B, 32, 32, 32, 5 + B)).max() > 0


def test_weight_gradient_is_exact_with_a_ragged_last_slab(ssd, cuda):
    """B = 3 on 10 x 14: R = 105 rows.  24 channels: rpp = 42, one slab of 336 rows with 105 in it (lanes of 3 and 2 rows); 32
    channels: one slab of 256; 8 channels: rpp = 128, one slab of 1024 -- 23 row lanes without a row; 4 channels: rpp = 256, one slab
    of 2048 -- 151 lanes without a row.  And three slabs, the last with 2 rows: 2 frames of 2 x 514 at 32 channels, R = 514 =
    256 + 256 + 2."""
    for Cout, plan in ((24, (42, 336, 1)), (32, (32, 256, 1)), (8, (128, 1024, 1)), (4, (256, 2048, 1))):
        assert uref.slab_plan(105, Cout) == plan
        assert np.abs(_exact_case(ssd, cuda, 3, 10, 14, Cout, 6 + Cout)).max() > 0
    assert uref.slab_plan(514, 32) == (32, 256, 3)
    assert np.abs(_exact_case(ssd, cuda, 2, 2, 514, 32, 9)).max() > 0


@pytest.mark.parametrize("Cout", [24, 32])
def test_weight_gradient_obeys_the_bound_of_a_double_sum_rounded_once(ssd, cuda, Cout):
    """Full-mantissa frames, normal dy: |dw - fl32(exact sum)| <= n 2^-53 sum|term| + one float32 ulp per element
    (head_train_ref.double_sum_bound, the uint8 test's bound): q and dy are floats, so the products are exact in double and only
    the order of the double additions and one rounding remain.  Two calls give the same bits; a workspace pre-filled with NaN
    changes nothing; the NaN pre-fill of dw is overwritten."""
    rng = np.random.default_rng(Cout)
    for H, W in [(10, 14), (32, 32)]:
        img = ref.full_mantissa_frames(rng, 3, H, W)
        dy = rng.normal(0, 1, (3, H // 2, W // 2, Cout)).astype(f32)
        terms = ref.fc_terms(img, dy)
        dw = _dw(ssd, cuda, img, dy)
        assert np.isfinite(dw).all() and np.abs(dw).max() > 0             # the NaN pre-fill is fully overwritten
        worst = 0.0
        for t in range(27):
            want, tol = href.double_sum_bound(terms[:, t, :])
            err = np.abs(dw.reshape(27, Cout)[t].astype(f64) - want.astype(f64))
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (H, W, t, float((err / tol).max()))
        print("first conv f32 dw Cout=%d %dx%d: worst |dw - exact| / bound = %.3g" % (Cout, H, W, worst))
        assert same_bits(dw, _dw(ssd, cuda, img, dy))
        assert same_bits(dw, _dw(ssd, cuda, img, dy, fill_ws=0xFF))       # 0xFF bytes: every double of the workspace a NaN


def test_the_last_row_and_column_matter(ssd, cuda):
    """A float at [b, H-1, W-1, ci] is seen by tap (1,1) of the last output only; one at [b, H-2, W-2, ci] by ky = 0 / kx = 0 of the
    last output row / column and ky = 2 / kx = 2 of the ones before.  dy has no zero, so every tap that can see the value moves; the
    kernel equals the exact reference (frames on the 2^-12 grid) before and after."""
    rng = np.random.default_rng(11)
    B, H, W, Cout = 2, 10, 14, 8
    img = ref.grid_frames(rng, B, H, W)
    dy = rng.choice(np.array([-3, -2, -1, 1, 2, 3], f32), (B, H // 2, W // 2, Cout))
    exact = lambda im: ref.fc_terms(im, dy).sum(0).reshape(3, 3, 3, Cout).astype(f32)
    other = lambda v: f32(0.75) if v != f32(0.75) else f32(0.25)
    base = _dw(ssd, cuda, img, dy)
    assert same_bits(base, exact(img))
    ci = 1
    corner = img.copy()
    corner[1, H - 1, W - 1, ci] = other(corner[1, H - 1, W - 1, ci])
    got = _dw(ssd, cuda, corner, dy)
    assert same_bits(got, exact(corner))
    moved = np.argwhere(got != base)
    assert len(moved) == Cout and all(tuple(m[:3]) == (1, 1, ci) for m in moved)
    above = img.copy()
    above[0, H - 2, W - 2, ci] = other(above[0, H - 2, W - 2, ci])
    got = _dw(ssd, cuda, above, dy)
    assert same_bits(got, exact(above))
    moved = {tuple(m[:3]) for m in np.argwhere(got != base)}
    assert moved == {(0, 0, ci), (0, 2, ci), (2, 0, ci), (2, 2, ci)}


# ----------------------------------------------------------------------------- 3. the byte grid, kernel level
@pytest.mark.parametrize("Cout", [24, 32])
def test_on_byte_grid_frames_the_calls_are_the_uint8_calls_bit_for_bit(ssd, cuda, Cout):
    """x = fp32(u * inv255): q(x) == p(u) (test_first_conv_f32_host.py), the same fmaf chain and the same slab order, so the forward
    and dw have the bits of ssd_first_conv_train_forward / _backward on the bytes."""
    rng = np.random.default_rng(30 + Cout)
    B = 3
    for H, W in [(10, 14), (32, 32)]:
        u = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        u[:, H - 1], u[:, :, W - 1] = 255, 0
        x = ref.byte_frames(u)
        k = rng.normal(0, 0.5, (3, 3, 3, Cout)).astype(f32)
        dy = rng.normal(0, 1, (B, H // 2, W // 2, Cout)).astype(f32)
        U, K, DY = cuda.from_numpy(u).cuda(), _dev(cuda, k), _dev(cuda, dy)
        want_y = cuda.full((B, H // 2, W // 2, Cout), float("nan"), device="cuda")
        ssd.train_calls.first_conv_forward(U, K, want_y)
        assert same_bits(_fwd(ssd, cuda, x, k), want_y.cpu().numpy()), (H, W)
        want_dw = fc_backward_dev(ssd, cuda, U, DY).cpu().numpy()
        assert same_bits(_dw(ssd, cuda, x, dy), want_dw) and np.abs(want_dw).max() > 0, (H, W)
        # and through the op with its autograd Function
        Kf, Ku = K.clone().requires_grad_(), K.clone().requires_grad_()
        yf, yu = ssd.first_conv_train_float(_dev(cuda, x), Kf), ssd.first_conv_train(U, Ku)
        assert cuda.equal(yf, yu)
        yf.backward(DY)
        yu.backward(DY)
        assert same_bits(Kf.grad.cpu().numpy(), want_dw) and same_bits(Ku.grad.cpu().numpy(), want_dw)


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_come_before_any_launch(ssd, cuda):
    L = ssd.lib()
    B, H, W, C = 2, 6, 8, 8
    img = cuda.zeros((B, H, W, 3), device="cuda")
    w = cuda.zeros((3, 3, 3, C), device="cuda")
    dy = cuda.zeros((B, H // 2, W // 2, C), device="cuda")
    out, dw = cuda.full((B, H // 2, W // 2, C), 7.0, device="cuda"), cuda.full((3, 3, 3, C), 7.0, device="cuda")
    ws = cuda.empty(1 << 20, dtype=cuda.uint8, device="cuda")
    s = ssd.train_calls.stream(img.device)
    need = L.ssd_first_conv_f32_train_workspace_bytes(B, H, W, C)
    assert 0 < need <= ws.numel()

    def fwd(b=B, h=H, ww=W, c=C, ip=img.data_ptr(), wp=w.data_ptr(), op=out.data_ptr()):
        return L.ssd_first_conv_f32_train_forward(ip, b, h, ww, wp, c, op, s)

    def bwd(b=B, h=H, ww=W, c=C, ip=img.data_ptr(), dyp=dy.data_ptr(), dwp=dw.data_ptr(), wsp=ws.data_ptr(), wsb=ws.numel()):
        return L.ssd_first_conv_f32_train_backward(ip, dyp, b, h, ww, c, dwp, wsp, wsb, s)
    sized = L.ssd_first_conv_f32_train_workspace_bytes
    for what, kw, word in (("odd H", dict(h=5), b"even"), ("odd W", dict(ww=7), b"even"),
                           ("Cout = 6", dict(c=6), b"Cout"), ("Cout = 68", dict(c=68), b"Cout"), ("Cout = 0", dict(c=0), b"Cout"),
                           ("B = 0", dict(b=0), b"positive"), ("H = 0", dict(h=0), b"positive"), ("W = -2", dict(ww=-2), b"positive"),
                           ("2^31 bytes", dict(b=313, h=640, ww=896), b"2^31")):
        assert fwd(**kw) == -1 and word in L.ssd_last_error(), what
        assert bwd(**kw) == -1 and word in L.ssd_last_error(), what
        assert sized(kw.get("b", B), kw.get("h", H), kw.get("ww", W), kw.get("c", C)) == 0, what
    for kw in (dict(ip=None), dict(wp=None), dict(op=None)):
        assert fwd(**kw) == -1 and b"null" in L.ssd_last_error(), kw
    for kw in (dict(ip=None), dict(dyp=None), dict(dwp=None), dict(wsp=None)):
        assert bwd(**kw) == -1 and b"null" in L.ssd_last_error(), kw
    for kw in (dict(ip=img.data_ptr() + 8), dict(wp=w.data_ptr() + 4), dict(op=out.data_ptr() + 8)):
        assert fwd(**kw) == -1 and b"16-byte" in L.ssd_last_error(), kw
    for kw in (dict(ip=img.data_ptr() + 4), dict(dyp=dy.data_ptr() + 4), dict(dwp=dw.data_ptr() + 4), dict(wsp=ws.data_ptr() + 8)):
        assert bwd(**kw) == -1 and b"16-byte" in L.ssd_last_error(), kw
    assert bwd(wsb=need - 1) == -1 and b"workspace too small" in L.ssd_last_error()
    cuda.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dw == 7.0).all())         # nothing ran
    assert fwd() == 0 and bwd(wsb=need) == 0                            # and the same calls with good arguments run
    cuda.cuda.synchronize()
    assert bool((out == 0).all()) and bool((dw == 0).all())
    # the op: a kernel on the GPU whose images are not, and the other way round; uint8 images stay first_conv_train's
    with pytest.raises(TypeError, match="GPU"):
        ssd.first_conv_train_float(img.cpu(), w)
    with pytest.raises(TypeError, match="GPU"):
        ssd.first_conv_train_float(img, w.cpu())
    with pytest.raises(TypeError, match="float32"):
        ssd.first_conv_train_float(img.to(cuda.uint8), w)
    with pytest.raises(TypeError, match="uint8"):
        ssd.first_conv_train(img, w)


# ----------------------------------------------------------------------------- 5. the modules
B = 2
NETS = {"mobilenet": (TINY_PARAMS, "TrainableMobileNet", ((16, 256), (8, 512), (4, 1024))),
        "shufflenet": (SN_PARAMS, "TrainableShuffleNet", ((16, 116), (8, 232), (4, 1024)))}
_shared = {}


def _setup(ssd, cuda, net):
    """Per backbone, computed once and left unchanged: the weights, the uint8 frames u, the float frames u * inv255, the engine's c3,
    c4, c5 on u and the upstream gradients."""
    if net not in _shared:
        params, _cls, outs = NETS[net]
        seed = {"mobilenet": 161, "shufflenet": 171}[net]
        W = ssd.synthetic_weights(params, seed=seed, logits_bias=-4.0)
        u = np.random.default_rng(seed + 1).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
        eng = ssd.Engine(params, W, device=0)
        eng.forward(cuda.from_numpy(u).cuda())
        kept = {k: eng.get_tensor(k) for k in ("c3", "c4", "c5")}
        eng.close()
        rng = np.random.default_rng(seed + 2)
        ds = [rng.normal(0, 1, (B, h, h, c)).astype(f32) for h, c in outs]
        _shared[net] = (W, u, ref.byte_frames(u), kept, ds)
    return _shared[net]


@pytest.mark.parametrize("train_first", [True, False])
@pytest.mark.parametrize("net", ["mobilenet", "shufflenet"])
def test_modules_on_byte_grid_float_frames_have_the_bits_of_the_uint8_frames(ssd, cuda, net, train_first):
    """The same module fed u and fed fp32(u * inv255): c3, c4, c5, every gradient and every moving statistic in .train(), c3, c4, c5
    in .eval() -- where both are the engine's.  The uint8 module is the parent's code, pinned by its own tests."""
    params, cls, _ = NETS[net]
    W, u, x, kept, ds = _setup(ssd, cuda, net)
    U, X = cuda.from_numpy(u).cuda(), _dev(cuda, x)
    D = [_dev(cuda, d) for d in ds]
    runs = {}
    for kind, frames in (("uint8", U), ("float32", X)):
        m = getattr(ssd, cls)(params, W, device="cuda", train_first=train_first).train()
        frozen = m.frozen_variables()
        assert len(frozen) == (0 if train_first else 5)
        names = set(m.named_variables())
        x0 = m.first_conv(frames)
        assert x0.requires_grad == train_first                           # frozen: the next layer is asked for no data gradient
        m = getattr(ssd, cls)(params, W, device="cuda", train_first=train_first).train()      # fresh statistics
        cs = m(frames)
        cuda.autograd.backward(cs, D)
        train = ([c.detach().cpu().numpy() for c in cs], {k: v.grad.cpu().numpy() for k, v in m.named_variables().items()},
                 {k: v.cpu().numpy() for k, v in m.statistics().items()})
        with cuda.no_grad():
            ev = [c.cpu().numpy() for c in m.eval()(frames)]
        assert set(m.named_variables()) == names and not (set(frozen) & (names | set(m.statistics())))
        for k, v in m.frozen_variables().items():                        # the frozen arrays: out of the variables, untouched
            assert same_bits(v, W[k]) and same_bits(frozen[k], W[k]), k
        if not train_first and kind == "float32":
            for k, v in m._frozen_on(X.device).items():
                assert same_bits(v.cpu().numpy(), W[k]) and not v.requires_grad, k
        runs[kind] = (train, ev, m)
    (tu, eu, mu), (tf, ef, mf) = runs["uint8"], runs["float32"]
    for l in range(3):
        assert same_bits(tf[0][l], tu[0][l]) and np.abs(tu[0][l]).max() > 0, l
        assert same_bits(ef[l], eu[l]), l
    assert set(tf[1]) == set(tu[1]) and set(tf[2]) == set(tu[2])
    for k in tu[1]:
        assert same_bits(tf[1][k], tu[1][k]), k
    for k in tu[2]:
        assert same_bits(tf[2][k], tu[2][k]) and not np.array_equal(tu[2][k], W[k]), k
    # .eval() on untouched statistics is the engine's c3, c4, c5
    m = getattr(ssd, cls)(params, W, device="cuda", train_first=train_first).eval()
    with cuda.no_grad():
        cs = m(X)
    for name, c in zip(("c3", "c4", "c5"), cs):
        assert np.array_equal(c.cpu().numpy(), kept[name]) and np.abs(kept[name]).max() > 0, name
    for k, v in m.statistics().items():
        assert same_bits(v.cpu().numpy(), W[k]), k


@pytest.mark.parametrize("net", ["mobilenet", "shufflenet"])
def test_modules_refuse_other_dtypes_and_channels_first(ssd, cuda, net):
    params, cls, _ = NETS[net]
    W = _setup(ssd, cuda, net)[0]
    m = getattr(ssd, cls)(params, W, device="cuda")
    with pytest.raises(TypeError, match="uint8 or float32"):
        m(cuda.zeros((1, 128, 128, 3), dtype=cuda.float64, device="cuda"))
    with pytest.raises(TypeError, match="uint8 or float32"):
        m(cuda.zeros((1, 128, 128, 3), dtype=cuda.float16, device="cuda"))
    with pytest.raises(TypeError, match=r"\[B,H,W,3\]"):
        m(cuda.zeros((1, 3, 128, 128), device="cuda"))                   # channels first
    with pytest.raises(TypeError, match="GPU"):
        m(cuda.zeros((1, 128, 128, 3)))
