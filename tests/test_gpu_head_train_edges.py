"""The TRAIN head at its edges (include/ssd_hip.h, "the TRAIN head").  The batch norm's out and dx bit for bit against the header's
float32 operation sequence, its statistics within one ulp of their float64 definitions, dgamma / dbeta within the derived bound
of a double sum rounded once -- at production row counts, at channel counts that leave lanes idle, over eight levels, in
inference mode, and on constant, dead, offset and poisoned channels.  The 3x3 convolution over class-count widths, widths beside
the tile edges, B = 1 and 3, thin levels, fewer rows than one K-step, eight levels and slice edges.  The predictor in training
mode on a 320 x 448 pyramid with B = 3.  Every tolerance is 0 or a bound derived in tests/helpers/head_train_ref.py; the one
exception is the predictor's FACTOR = 4, the project's margin.  Measured figures: profiles/r15_head_train_edges.log."""
import numpy as np
import pytest

from helpers import head_train_ref as ref
from helpers.head_train_gpu import bn_raw, conv_backward, conv_backward_raw, dev, predictor_training_check, same_bits, ulps
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
LP = {"gamma": 2.0, "alpha": 0.25}
SMALL_OFFSET = 16.0         # |mean| / std up to which the variance is ALSO compared with the one around the true mean: the two
                            # differ by (mean32 - mean)^2 <= (2^-24 mean)^2, i.e. (2^-24 * 16)^2 = 2^-40 of the variance there,
                            # 2^-16 of its float32 rounding


def _bn_inputs(rng, rows, C, mean=0.3, std=1.5):
    xs = [rng.normal(mean, std, (r, C)).astype(f32) for r in rows]
    dys = [rng.normal(0, 1, (r, C)).astype(f32) for r in rows]
    gammas = [rng.uniform(0.5, 1.5, C).astype(f32) for _ in rows]
    betas = [rng.normal(0, 0.3, C).astype(f32) for _ in rows]
    mms = [rng.normal(0, 0.1, C).astype(f32) for _ in rows]
    mvs = [rng.uniform(0.5, 1.5, C).astype(f32) for _ in rows]
    return xs, gammas, betas, mms, mvs, dys


def _check_bn(ssd, cuda, tag, xs, gammas, betas, mms, mvs, dys, skip=()):
    """Every assertion of the module docstring on one call; `skip`: channels with non-finite data (compared by the caller).
    Returns the kernel's outputs."""
    got = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)
    again = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)
    C = xs[0].shape[-1]
    keep = np.setdiff1d(np.arange(C), np.asarray(skip, np.int64))
    for i, g in enumerate(got):
        x, dy = xs[i].reshape(-1, C)[:, keep], dys[i].reshape(-1, C)[:, keep]
        gamma, beta = gammas[i][keep], betas[i][keep]
        k = {name: (v.reshape(-1, C)[:, keep] if v.ndim > 1 else v[keep]) for name, v in g.items()}
        R = x.shape[0]
        x64 = x.astype(f64)
        mean64 = x64.mean(0)
        assert ulps(k["mean"], mean64.astype(f32)).max() <= 1
        # the header's variance: around the kernel's OWN float32 mean, difference and square in double, rounded once
        var64 = ((x64 - k["mean"].astype(f64)) ** 2).mean(0)
        assert ulps(k["var"], var64.astype(f32)).max() <= 1
        true64 = ((x64 - mean64) ** 2).mean(0)
        small = np.abs(mean64) <= SMALL_OFFSET * np.sqrt(true64)
        assert ulps(k["var"][small], true64[small].astype(f32)).max(initial=0) <= 1
        del x64
        assert same_bits(k["invstd"], ref.invstd_f32(k["var"]))
        mm, mv = ref.moving_update(mms[i][keep], mvs[i][keep], k["mean"], k["var"], R)
        assert same_bits(k["mm"], mm) and same_bits(k["mv"], mv)
        assert same_bits(k["y"], ref.bn_relu_f32(x, gamma, beta, k["mean"], k["var"])), (tag, i)
        gate, xhat = ref.bn_gate_f32(x, gamma, beta, k["mean"], k["var"], dy)
        dist = {}
        for name, terms in (("dbeta", gate.astype(f64)), ("dgamma", gate.astype(f64) * xhat.astype(f64))):
            want, tol = ref.double_sum_bound(terms)
            err = np.abs(k[name].astype(f64) - want.astype(f64))
            dist[name] = ulps(k[name], want).max()
            assert np.all(err <= tol), (tag, i, name, float((err / tol).max()))
        _, dx, _, _ = ref.bn_relu_f32(x, gamma, beta, k["mean"], k["var"], dy, dgamma=k["dgamma"], dbeta=k["dbeta"])
        assert same_bits(k["dx"], dx), (tag, i)
        print("batch norm %s level %d (%d rows x %d): dgamma %d ulp, dbeta %d ulp from the exact sum rounded once" % (tag, i, R, C, dist["dgamma"], dist["dbeta"]))
        for name in g:                                                   # two runs, the same bits (poisoned channels included)
            assert same_bits(g[name], again[i][name]), (tag, i, name)
    return got


def test_batch_norm_at_production_row_counts(ssd, cuda):
    """16 images of 640 x 896: 143 360 + 35 840 + 8 960 + 2 240 + 560 rows of 256 channels.  slab_rows leaves its floor (188) and
    the call has 1 017 slabs, every level's last one partial."""
    rows, C = [143360, 35840, 8960, 2240, 560], 256
    rpp, slab_rows, n_slabs = ref.slab_plan(rows, C)
    assert (rpp, slab_rows, n_slabs) == (4, 188, 1017) and all(r % slab_rows for r in rows)
    assert ssd.train_calls.bn_workspace_bytes(rows, C) == ref.al256(1017 * 2 * 256 * 8)
    _check_bn(ssd, cuda, "production", *_bn_inputs(np.random.default_rng(1), rows, C))


# C: (rows per level, rpp, slab_rows): several slabs and a partial last one in the larger levels, a one-row level at the end
CHANNELS = {6: ([5000, 1030, 1], 128, 1024), 20: ([1500, 409, 1], 51, 408), 100: ([700, 81, 1], 10, 80), 516: ([100, 9, 1], 1, 8),
            1024: ([100, 9, 1], 1, 8)}


@pytest.mark.parametrize("C", sorted(CHANNELS))
def test_batch_norm_channel_counts(ssd, cuda, C):
    """C = 6 and 20: the element-wise path is not taken by 20 (a multiple of 4) but its 5 quads leave one thread of 256 idle and
    rpp = 51 divides nothing; 6 takes the element-wise loads with rpp = 128; 100: rpp = 10, 6 idle threads; 516: rpp = 1, 127 idle
    threads; 1024: every thread a quad, rpp = 1."""
    rows, rpp, slab_rows = CHANNELS[C]
    got = ref.slab_plan(rows, C)
    assert got[:2] == (rpp, slab_rows), got
    assert rows[0] > 2 * slab_rows and rows[0] % slab_rows and rows[1] > slab_rows and rows[1] % slab_rows
    _check_bn(ssd, cuda, "C=%d" % C, *_bn_inputs(np.random.default_rng(C), rows, C))


def test_batch_norm_eight_levels_and_no_more(ssd, cuda):
    rows, C = [442, 126, 99, 40, 33, 12, 2, 1], 256
    assert len(rows) == 8
    data = _bn_inputs(np.random.default_rng(8), rows, C)
    _check_bn(ssd, cuda, "eight levels", *data)
    # nine levels are refused by every entry point (before any HIP call)
    L, Lv = ssd.lib(), ssd._lib.SsdBnLevel
    x = dev(cuda, data[0][0])
    nine = (Lv * 9)(*[Lv(442, *([x.data_ptr()] * 12)) for _ in range(9)])
    assert L.ssd_bn_relu_train_workspace_bytes(nine, 9, C) == 0
    ws = cuda.empty(1 << 20, dtype=cuda.uint8, device="cuda")
    assert L.ssd_bn_relu_train_forward(nine, 9, C, 1, 1e-3, 0.007, ws.data_ptr(), ws.numel(), None) == -1
    assert b"1 .. 8 levels" in L.ssd_last_error()
    assert L.ssd_bn_relu_train_backward(nine, 9, C, ws.data_ptr(), ws.numel(), None) == -1
    assert b"1 .. 8 levels" in L.ssd_last_error()


@pytest.mark.parametrize("C", [256, 6])
def test_batch_norm_inference_mode_through_the_raw_entry_point(ssd, cuda, C):
    """training = 0: out = max(((x - moving_mean) * (gamma * (1 / sqrt(moving_variance + epsilon)))) + beta, 0) bit for bit; mean, var,
    invstd and the moving statistics are not written (a sentinel stays); a NULL workspace is accepted."""
    rows = [442, 35, 1]
    xs, gammas, betas, mms, mvs, _ = _bn_inputs(np.random.default_rng(C + 1), rows, C)
    SENTINEL = -123.25
    got = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, training=0, fill=SENTINEL, workspace=False)
    for i, g in enumerate(got):
        want = ref.bn_relu_f32(xs[i], gammas[i], betas[i], mms[i], mvs[i])          # the same expression on the moving statistics
        assert same_bits(g["y"], want) and np.abs(want).max() > 0
        for name in ("mean", "var", "invstd"):
            assert np.all(g[name] == f32(SENTINEL)), name
        assert same_bits(g["mm"], mms[i]) and same_bits(g["mv"], mvs[i])


CONSTANT, DEAD, OFFSET, POISON = (3, 4, 5), (40, 41, 42), (100, 101, 102), (200, 201)


def _degenerate_inputs():
    rng = np.random.default_rng(5)
    C, rows = 256, [442]
    xs, gammas, betas, mms, mvs, dys = _bn_inputs(rng, rows, C)
    for c, v in zip(CONSTANT, (0.75, 3.0, -2.5)):                         # rows * v and every partial sum are exact in double
        xs[0][:, c] = v
    betas[0][list(CONSTANT)] = [0.25, -0.5, 0.125]
    betas[0][list(DEAD)] = -100.0
    for c in OFFSET:
        xs[0][:, c] = (1e3 + 1e-2 * rng.normal(0, 1, rows[0])).astype(f32)
    return xs, gammas, betas, mms, mvs, dys


def test_batch_norm_degenerate_statistics(ssd, cuda):
    """Constant channels (variance exactly 0), channels whose ReLU is dead everywhere, and channels with mean 1e3 and std 1e-2.
    The offset channels separate the header's two-pass variance from a one-pass one: around the float32 mean the sum is off the
    true variance by (mean32 - mean)^2 <= (ulp(1e3) / 2)^2 = 9e-10, 1e-5 of the variance 1e-4 (bound 2 ulp^2 / var = 7.5e-5), while
    a one-pass E[x^2] - mean32^2 is off by 2 * mean * (mean32 - mean), up to 0.06: six hundred times the variance itself, seven
    orders of magnitude outside the bound (tests/test_head_train_host.py shows both on the CPU)."""
    xs, gammas, betas, mms, mvs, dys = _degenerate_inputs()
    g = _check_bn(ssd, cuda, "degenerate", xs, gammas, betas, mms, mvs, dys)[0]
    R = 442
    c = list(CONSTANT)
    assert same_bits(g["mean"][c], np.array([0.75, 3.0, -2.5], f32)) and same_bits(g["var"][c], np.zeros(3, f32))
    # the header's invstd is two float32 operations, 1 / sqrt(0 + eps): one ulp below fp32(1 / sqrt(eps)) rounded once
    assert same_bits(g["invstd"][c], ref.invstd_f32(np.zeros(3, f32)))
    assert ulps(g["invstd"][c], np.full(3, 1.0 / np.sqrt(float(f32(ref.EPS))), f32)).max() <= 1
    assert same_bits(g["y"][:, c], np.broadcast_to(np.maximum(betas[0][c], f32(0)), (R, 3)))
    assert np.all(g["dgamma"][c] == 0)
    assert g["dbeta"][c[1]] == 0 and np.all(g["dbeta"][[c[0], c[2]]] != 0)           # beta -0.5: the gate is closed; 0.25, 0.125: open
    assert np.all(g["mv"][c] < mvs[0][c]) and np.all(g["mv"][c] > 0)                  # the moving variance moves toward 0
    d = list(DEAD)
    assert np.all(g["y"][:, d] == 0) and np.all(g["dgamma"][d] == 0) and np.all(g["dbeta"][d] == 0)
    assert np.all(g["dx"][:, d] == 0)                                                 # +0 or -0
    o = list(OFFSET)
    x64 = xs[0][:, o].astype(f64)
    true = ((x64 - x64.mean(0)) ** 2).mean(0)
    assert np.all(np.abs(x64.mean(0)) > 1e4 * np.sqrt(true))                          # far outside SMALL_OFFSET
    bound = ref.offset_variance_bound(1e3, true.max())
    relerr = np.abs(g["var"][o].astype(f64) - true) / true
    print("offset channels: var off the true variance by %s relative (bound %.3g)" % (relerr, bound))
    assert np.all(relerr <= bound)


@pytest.mark.parametrize("where", ["x", "dy"])
def test_batch_norm_poisoned_channels_stay_alone(ssd, cuda, where):
    """One NaN in channel 200 and one +Inf in channel 201, in x or in dy (there at a row whose gate is open): the columns are
    independent, so EVERY other channel's y, statistics, dx, dgamma and dbeta keep their bits.  In the poisoned channels every
    output that the poison reaches is non-finite, with one exception that the header defines: max(v, 0) is v > 0 ? v : 0 here as in
    every ReLU of the library, so a NaN pre-activation gives y = 0 and a closed gate (g = 0, dbeta = 0); with the poison in x the
    statistics (NaN) say so, and dgamma and dx are NaN."""
    xs, gammas, betas, mms, mvs, dys = _degenerate_inputs()
    clean = bn_raw(ssd, cuda, xs, gammas, betas, mms, mvs, dys)[0]
    p = list(POISON)
    row = int(np.argmax((clean["y"][:, p[0]] > 0) & (clean["y"][:, p[1]] > 0)))
    assert clean["y"][row, p[0]] > 0 and clean["y"][row, p[1]] > 0
    target = xs if where == "x" else dys
    target[0][row, p[0]], target[0][row, p[1]] = np.nan, np.inf
    g = _check_bn(ssd, cuda, "poison in " + where, xs, gammas, betas, mms, mvs, dys, skip=POISON)[0]
    others = np.setdiff1d(np.arange(256), p)
    for name in g:
        a, b = (g[name][:, others], clean[name][:, others]) if g[name].ndim > 1 else (g[name][others], clean[name][others])
        assert same_bits(a, b), name
    if where == "x":
        for name in ("mean", "var", "invstd", "mm", "mv", "dgamma"):
            assert not np.isfinite(g[name][p]).any(), name
        assert not np.isfinite(g["dx"][:, p]).any()
        assert np.all(g["y"][:, p] == 0) and np.all(g["dbeta"][p] == 0)           # the header's ReLU and gate on a NaN
    else:
        for name in ("mean", "var", "invstd", "mm", "mv"):
            assert same_bits(g[name][p], clean[name][p]), name
        assert same_bits(g["y"][:, p], clean["y"][:, p])
        assert not np.isfinite(g["dgamma"][p]).any() and not np.isfinite(g["dbeta"][p]).any()
        assert not np.isfinite(g["dx"][:, p]).any()


# ----------------------------------------------------------------------------- the convolution
@pytest.mark.parametrize("case", sorted(ref.CONV_CASES))
def test_convolution_sweep(ssd, cuda, oracle_ops, case):
    """Per case of helpers.head_train_ref.CONV_CASES: the forward bit-identical to ssd_conv2d with and without bias; dx bit-identical
    to the oracle's conv2d(dy, w'); dw and dbias EXACT on small integers (the premise asserted); dw on random data within the
    order-free bound gamma_n * sum|x * dy|, dbias a double sum rounded once, two runs the same bits."""
    B, sizes, Cin, Cout = ref.CONV_CASES[case]
    rows = [B * h * w for h, w in sizes]
    rps = ref.rows_per_slice(rows, Cin, Cout)
    if case == "slice-edge":
        assert rows[0] == 2 * rps and rows[1] == 2 * rps + 1
    if case == "six-rows":
        assert sum(rows) < 16
    if case == "eight-levels":
        assert len(sizes) == 8
    if case == "264-132":
        assert -(-Cin // 128) == 3 and Cin - 256 == 8
    _, _, xs, w, bias, dys = ref.conv_case_data(case, integers=False)
    for b in (None, bias):
        ys = ssd.conv3x3_same([dev(cuda, x) for x in xs], dev(cuda, w), None if b is None else dev(cuda, b))
        for x, y in zip(xs, ys):
            want = ssd.ssd.conv2d(dev(cuda, x), w, bias=b)
            assert y.shape == want.shape and cuda.equal(y, want), (x.shape, b is None)
    dxs, dw, db = conv_backward(ssd, cuda, xs, w, dys)
    wr = ref.rotated_transposed(w)
    for dy, dx in zip(dys, dxs):
        assert np.array_equal(dx, oracle_ops.conv2d(dy, wr)), dy.shape
    dw64, bound, absum = ref.wgrad_bound(xs, w, dys)
    err = np.abs(dw.astype(f64) - dw64)
    print("wgrad %s (%d -> %d, %d rows, slices of %d): max |dw - dw64| / bound = %.3g" % (case, Cin, Cout, sum(rows), rps, (err / bound).max()))
    assert np.all(err <= bound)
    want, tol = ref.double_sum_bound(np.concatenate([d.reshape(-1, Cout) for d in dys]).astype(f64))
    assert np.all(np.abs(db.astype(f64) - want.astype(f64)) <= tol)
    _, dw2, db2 = conv_backward(ssd, cuda, xs, w, dys)
    assert same_bits(dw, dw2) and same_bits(db, db2)
    # integers: exact in any order
    _, _, xs, w, _, dys = ref.conv_case_data(case, integers=True)
    dw64, db64, top_w, top_b = ref.integer_premise(xs, w, dys)
    assert top_w < 2 ** 24 and top_b < 2 ** 24 and np.abs(dw64).max() > 0
    _, dw, db = conv_backward(ssd, cuda, xs, w, dys)
    assert np.array_equal(dw.astype(f64), dw64) and np.array_equal(db.astype(f64), db64)


@pytest.mark.parametrize("case", ["256-18", "72-33", "eight-levels"])
def test_backward_without_dx_and_without_dbias(ssd, cuda, case):
    """The raw entry point with out == NULL for every level: dw and dbias have the bits of the call that also produces dx; with
    dbias_dev == NULL the (sentinel-filled) buffer is not touched and dw is the same again."""
    _, _, xs, w, _, dys = ref.conv_case_data(case, integers=False)
    SENTINEL = -7.5
    dxs, dw, db = conv_backward_raw(ssd, cuda, xs, w, dys, True, True, SENTINEL)
    none, dw1, db1 = conv_backward_raw(ssd, cuda, xs, w, dys, False, True, SENTINEL)
    assert none is None and same_bits(dw, dw1) and same_bits(db, db1)
    Cout = w.shape[3]
    assert np.isfinite(dw).all() and np.isfinite(db[:Cout]).all() and not np.any(db[:Cout] == f32(SENTINEL))
    assert np.all(db[Cout:] == f32(SENTINEL))                                        # nothing past Cout is written
    _, dw2, db2 = conv_backward_raw(ssd, cuda, xs, w, dys, False, False, SENTINEL)
    assert same_bits(dw, dw2) and np.all(db2 == f32(SENTINEL))
    ax, aw, ab = conv_backward(ssd, cuda, xs, w, dys)                                # the autograd path is the same call
    assert same_bits(aw, dw) and same_bits(ab, db[:Cout]) and all(same_bits(a, b) for a, b in zip(ax, dxs))


@pytest.mark.parametrize("case", ["256-18", "72-33"])
def test_weight_gradient_rows_and_columns_are_independent(ssd, cuda, case):
    """One +Inf in input channel ci* of x: every dw[:, :, ci, :] with ci != ci* keeps its bits (and dbias all of them).  One +Inf in
    output channel co* of dy: every dw[..., co] and dbias[co] with co != co* keeps its bits.  The poisoned row / column itself is
    non-finite at the centre tap."""
    _, _, xs, w, _, dys = ref.conv_case_data(case, integers=False)
    Cin, Cout = w.shape[2], w.shape[3]
    _, dw, db = conv_backward(ssd, cuda, xs, w, dys)
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    ci, co = Cin - 3, Cout - 2
    px = [x.copy() for x in xs]
    px[0][1, 6, 8, ci] = np.inf
    _, dw1, db1 = conv_backward(ssd, cuda, px, w, dys)
    keep = np.arange(Cin) != ci
    assert same_bits(dw1[:, :, keep, :], dw[:, :, keep, :]) and same_bits(db1, db)
    assert not np.isfinite(dw1[1, 1, ci, :]).any()
    py = [d.copy() for d in dys]
    py[1][0, 3, 4, co] = np.inf
    _, dw2, db2 = conv_backward(ssd, cuda, xs, w, py)
    keep = np.arange(Cout) != co
    assert same_bits(dw2[..., keep], dw[..., keep]) and same_bits(db2[keep], db[keep])
    assert not np.isfinite(dw2[1, 1, :, co]).any() and not np.isfinite(db2[co])


# ----------------------------------------------------------------------------- the predictor
def test_predictor_in_training_mode_on_a_larger_non_square_pyramid(ssd, cuda):
    """tests/test_gpu_head_train.py's training-mode comparison (the same body: helpers.head_train_gpu.predictor_training_check) on
    B = 3 random normal feature maps of a 320 x 448 image, (40, 56) .. (3, 4): 8 961 rows against the 682 of the 128 x 128 run.
    The same reference (float64 restatement + float64 autograd of the loss), the same yardstick (float32 CPU torch), FACTOR = 4."""
    FACTOR = 4.0
    predictor_training_check(ssd, cuda, TINY_PARAMS, LP, *ref.large_predictor_input(ssd, TINY_PARAMS), factor=FACTOR, tag="320x448")
