"""ssd_train_histograms on the GPU against its numpy restatement (helpers/histogram_ref.py), bit for bit: tensor sizes around the block
size at every offset of w inside its 16-byte group, gradients of w's alignment class, of another one and NULL, decaying rows with a
weight_decay that moves elements into other buckets, the float32 neighbours of the limits, zeros, denormals, +-FLT_MAX, NaN and
infinities on the ends of a tensor and across a block boundary, constant and two-valued tensors (every lane of a wave on one LDS
address) under every aggregation scheme, a table with an empty tensor, outputs and workspace pre-filled with NaN bytes behind guard
words, the sums of squares against ssd_train_norms, the refusals with the outputs untouched, and TrainStep.histograms() after a real
backward of the head."""
import ctypes

import numpy as np
import pytest

from helpers import head_train_ref as href
from helpers import histogram_ref as ref
from helpers.head_train_gpu import dev as _dev
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
COUNTS = (1, 4095, 4096, 4097, 3 * 4096 + 5)
GUARD = 0x5A
NAN_BYTE = 0xFF                          # float64 / float32 of 0xFF bytes is a NaN, int64 is -1
WD = 0.5                                 # g + 0.5 * w lands in other buckets than g
FLT_MAX = np.finfo(f32).max


def _values(rng, n):
    """Random signs and mantissas over +-40 binades: the order of the additions shows in the last bits of the sums."""
    return (rng.normal(0, 1, n) * np.exp2(rng.integers(-40, 41, n))).astype(f32)


class _Arena:
    """Tensors at chosen float offsets from a 16-byte boundary inside one device buffer."""

    def __init__(self, cuda, floats):
        self.cuda = cuda
        self.buf = cuda.zeros(floats, dtype=cuda.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.at = 0

    def put(self, host, offset):
        start = (self.at + 3) // 4 * 4 + offset
        self.at = start + max(len(host), 1)
        view = self.buf[start:start + len(host)]
        if len(host):
            view.copy_(self.cuda.from_numpy(host))
        assert (self.buf.data_ptr() + 4 * start) % 16 == 4 * offset
        return view, self.buf.data_ptr() + 4 * start


def _table(cuda, specs):
    """specs: (w host array, grad host array or None, w offset, grad offset, decay) per row -> the arena, the rows (host uint8 tensor,
    device copy), the blocks and the restatement's input."""
    from ssd_amd import train_step
    arena = _Arena(cuda, sum(len(w) + 8 + (len(g) + 8 if g is not None else 0) for w, g, _a, _b, _d in specs) + 16)
    rows = np.zeros(len(specs), train_step.TENSOR_DTYPE)
    want = []
    for t, (w, g, wo, go, decay) in enumerate(specs):
        _wt, wp = arena.put(w, wo)
        gp = arena.put(g, go)[1] if g is not None else 0
        rows[t]["w"], rows[t]["grad"], rows[t]["count"] = wp, gp, len(w)
        rows[t]["m"] = rows[t]["v"] = rows[t]["ema"] = wp              # validated, never dereferenced
        rows[t]["decay"] = decay
        want.append((w, g, wo, decay))
    rows["first_block"], blocks = train_step.block_starts(rows["w"], rows["count"])
    host = cuda.from_numpy(rows.view(np.uint8).copy())
    return arena, host, host.cuda(), blocks, want


def _guarded(cuda, shape, dtype, guard_rows=1):
    """A tensor of `shape` pre-filled with NaN bytes between guard rows -> (the whole buffer as bytes, the inner view)."""
    full = cuda.empty((shape[0] + 2 * guard_rows,) + tuple(shape[1:]), dtype=dtype, device="cuda")
    raw = full.view(cuda.uint8)
    raw.fill_(GUARD)
    inner = full[guard_rows:guard_rows + shape[0]]
    inner.view(cuda.uint8).fill_(NAN_BYTE)
    return raw, inner


@pytest.fixture(scope="module")
def limits_dev(ssd, cuda):
    return cuda.from_numpy(ssd.histogram_limits().copy()).cuda()


def _host_stats(stats):
    from ssd_amd import train_calls
    return stats.cpu().numpy().view(train_calls.STATS_DTYPE)[:, :, 0]


def _compare(tag, counts, stats, want_c, want_s):
    wrong = np.nonzero(counts != want_c)
    assert len(wrong[0]) == 0, (tag, [w[:5] for w in wrong], counts[wrong][:5], want_c[wrong][:5])
    for field in ("num", "bad"):
        assert np.array_equal(stats[field], want_s[field]), (tag, field, np.nonzero(stats[field] != want_s[field]))
    for field, bits in (("sum", np.int64), ("sum_squares", np.int64), ("min", np.int32), ("max", np.int32)):
        a, b = np.ascontiguousarray(stats[field]).view(bits), np.ascontiguousarray(want_s[field]).view(bits)
        wrong = np.nonzero(a != b)
        assert len(wrong[0]) == 0, (tag, field, wrong, stats[field][wrong][:5], want_s[field][wrong][:5])
    assert stats.tobytes() == want_s.tobytes(), tag


def _run_and_check(ssd, cuda, limits_dev, specs, tag, weight_decay=WD):
    arena, host, devrows, blocks, want = _table(cuda, specs)
    calls = ssd.train_calls
    T, NB = len(specs), ref.NB
    need = calls.train_histograms_workspace_bytes(host)
    assert need == 64 * blocks
    craw, counts = _guarded(cuda, (T, 2, NB), cuda.int64)
    sraw, stats = _guarded(cuda, (T, 2, 40), cuda.uint8)
    wraw = cuda.full((need + 32,), GUARD, dtype=cuda.uint8, device="cuda")
    ws = wraw[16:16 + need]
    ws.fill_(NAN_BYTE)
    assert ws.data_ptr() % 16 == 0
    before = arena.buf.clone()
    calls.train_histograms(host, devrows, weight_decay, limits_dev, counts, stats, workspace=ws)
    c1, s1 = counts.cpu().numpy().copy(), _host_stats(stats).copy()
    counts.view(cuda.uint8).fill_(NAN_BYTE)
    stats.fill_(NAN_BYTE)
    calls.train_histograms(host, devrows, weight_decay, limits_dev, counts, stats, workspace=ws)
    c2, s2 = counts.cpu().numpy(), _host_stats(stats)
    want_c, want_s = ref.table_histograms(want, weight_decay)
    _compare(tag, c1, s1, want_c, want_s)
    assert np.array_equal(c1, c2) and s1.tobytes() == s2.tobytes(), tag                             # two calls, the same bytes
    assert cuda.equal(arena.buf.view(cuda.int32), before.view(cuda.int32)), tag                     # w and grad keep their bits
    for raw, row_bytes in ((craw, 2 * NB * 8), (sraw, 2 * 40)):
        r = raw.reshape(-1).cpu().numpy()
        assert (r[:row_bytes] == GUARD).all() and (r[-row_bytes:] == GUARD).all(), tag
    r = wraw.cpu().numpy()
    assert (r[:16] == GUARD).all() and (r[16 + need:] == GUARD).all(), tag
    assert (c1.sum(axis=2) == s1["num"]).all(), tag
    return c1, s1, (host, devrows, arena)


def _sweep_specs(rng):
    """Every count at every w offset, with a gradient of w's class, of another class, and NULL; decay alternates."""
    specs = []
    for n in COUNTS:
        for wo in range(4):
            specs.append((_values(rng, n), _values(rng, n), wo, wo, (n + wo) & 1))
            specs.append((_values(rng, n), _values(rng, n), wo, (wo + 1 + (n + wo) % 3) % 4, (n + wo + 1) & 1))
            specs.append((_values(rng, n), None, wo, 0, wo & 1))
    return specs


def test_sizes_offsets_gradient_classes_and_decay_in_one_table(ssd, cuda, limits_dev):
    specs = _sweep_specs(np.random.default_rng(0))
    assert len(specs) == 60
    c, s, _ = _run_and_check(ssd, cuda, limits_dev, specs, "sweep")
    assert not s["bad"].any() and (s["num"][:, 0] == [len(sp[0]) for sp in specs]).all()
    assert (s["num"][2::3, 1] == 0).all() and (s["num"][0::3, 1] > 0).all() and (s["num"][1::3, 1] > 0).all()
    # the decay term moved elements: a decaying row's gradient plane differs from the plane of the bare gradient
    moved = [t for t, (w, g, wo, _go, decay) in enumerate(specs)
             if g is not None and decay and len(w) > 1 and not np.array_equal(ref.plane(g, wo)[0], c[t, 1])]
    assert len(moved) >= 10


@pytest.mark.parametrize("n,wo,go,decay", [(1, 3, 3, 1), (4097, 1, 1, 1), (4097, 2, 0, 0), (3 * 4096 + 5, 0, None, 1), (4096, 3, 2, 1)])
def test_a_table_of_one_tensor(ssd, cuda, limits_dev, n, wo, go, decay):
    rng = np.random.default_rng(n + wo)
    _run_and_check(ssd, cuda, limits_dev, [(_values(rng, n), _values(rng, n) if go is not None else None, wo, go or 0, decay)], "T = 1")


def _edge_values():
    """The float32 neighbours of a spread of limits (two on either side, and the rounded limit itself), of both signs; zeros;
    denormals; +-FLT_MAX; powers of two over +-40 binades and beyond."""
    M = ref.NB // 2
    pos = ref.LIMITS[M + 1:-1]                                       # the finite positive limits
    picks = sorted(set([0, 1, 2, len(pos) - 1, len(pos) - 2] + list(range(0, len(pos), 37)) +
                       [int(np.searchsorted(pos, v)) for v in (1e-3, 1.0, 1e3, float(FLT_MAX))]))
    vals = []
    for k in picks:
        if k >= len(pos):
            continue
        with np.errstate(over="ignore"):
            f = f32(pos[k])
        if not np.isfinite(f):
            f = FLT_MAX
        lo1 = np.nextafter(f, f32(0))
        lo2 = np.nextafter(lo1, f32(0))
        hi1 = np.nextafter(f, f32(np.inf))
        hi2 = np.nextafter(hi1, f32(np.inf))
        for v in (lo2, lo1, f, hi1, hi2):
            if np.isfinite(v):
                vals += [v, -v]
    tiny = np.array([1, 2, 0x7fffff, 0x800000, 0x800001], np.uint32).view(f32)       # denormals, FLT_MIN and its neighbour
    vals += [f32(0.0), f32(-0.0), FLT_MAX, -FLT_MAX] + list(tiny) + list(-tiny)
    vals += [f32(2.0) ** e for e in range(-149, 128, 3)] + [-(f32(2.0) ** e) for e in range(-149, 128, 3)]
    return np.array(vals, f32)


def test_the_neighbours_of_the_limits_zeros_denormals_and_extremes(ssd, cuda, limits_dev):
    rng = np.random.default_rng(5)
    edge = _edge_values()
    assert len(edge) > 400 and np.isfinite(edge).all()
    specs = []
    for wo in range(4):
        w = rng.permutation(edge)
        g = rng.permutation(edge)
        specs.append((w, g, wo, (wo + wo // 2) % 4, 0))              # decay 0: the gradient plane is the edge values themselves
    specs.append((edge, edge.copy(), 1, 1, 1))                       # decay 1: FLT_MAX + 0.5 * FLT_MAX is +inf and counts as bad
    big = np.concatenate([rng.permutation(edge), _values(rng, 4096 * 2 - len(edge) + 3)])
    specs.append((big, rng.permutation(big), 2, 2, 0))
    c, s, _ = _run_and_check(ssd, cuda, limits_dev, specs, "edges")
    M = ref.NB // 2
    assert (s["bad"][:4] == 0).all() and (s["num"][:4] == len(edge)).all()
    assert (s["min"][:4] == -FLT_MAX).all() and (s["max"][:4] == FLT_MAX).all()
    # both zeros and every positive value below 1e-12 in bucket M + 1, every negative one above -1e-12 in bucket M
    assert c[0, 0, M + 1] == 2 + int(((edge > 0) & (edge.astype(f64) < 1e-12)).sum())
    assert c[0, 0, M] == int(((edge < 0) & (edge.astype(f64) > -1e-12)).sum())
    assert s["bad"][4, 1] > 0                                        # FLT_MAX + 0.5 * FLT_MAX


def test_non_finite_elements_on_the_ends_and_across_a_block_boundary(ssd, cuda, limits_dev):
    rng = np.random.default_rng(2)
    specs, planted = [], []
    for wo, go in ((0, 0), (1, 1), (3, 2), (2, 2)):
        n = 2 * 4096 + 7
        w, g = _values(rng, n), _values(rng, n)
        edge = 4096 - wo                                             # the element that opens the tensor's second block
        w[[0, n - 1]] = [np.nan, -np.inf]
        w[[edge - 1, edge]] = [np.inf, np.nan]
        g[[0, edge - 1, edge, n - 1]] = [np.inf, -np.inf, np.inf, np.nan]
        g[100] = np.nan
        specs.append((w, g, wo, go, 0))
        planted.append([4, 5])
    w = np.array([np.nan, np.inf, -np.inf], f32)                     # nothing finite
    specs.append((w, None, 1, 0, 0))
    planted.append([3, 0])
    w, g = _values(rng, 4100), _values(rng, 4100)                    # a decaying row: a bad w makes g' bad, too
    w[[0, 4099]] = [np.nan, np.inf]
    g[7] = -np.inf
    specs.append((w, g, 3, 3, 1))
    planted.append([2, 3])
    c, s, _ = _run_and_check(ssd, cuda, limits_dev, specs, "non-finite")
    assert s["bad"].tolist() == planted and np.isfinite(s["sum"]).all() and np.isfinite(s["sum_squares"]).all()
    assert np.isfinite(s["min"][:4]).all() and np.isfinite(s["max"][:4]).all()
    assert s["num"][4, 0] == 0 and s["min"][4, 0] == np.inf and s["max"][4, 0] == -np.inf and c[4].sum() == 0
    assert (c.sum(axis=2) + s["bad"] == [[len(sp[0]), len(sp[0]) if sp[1] is not None else 0] for sp in specs]).all()


@pytest.mark.parametrize("scheme", [None, 0, 1, 2, 3, 4])
def test_constant_and_two_valued_tensors_under_every_scheme(ssd, cuda, limits_dev, scheme):
    """A lost LDS or global atomic shows as a wrong count.  Every scheme of option "hist_scheme" gives the same bytes."""
    n = 5 * 4096
    rng = np.random.default_rng(9)
    two = np.where(rng.integers(0, 2, n) == 1, f32(0.75), f32(-3e-5)).astype(f32)
    striped = np.where(np.arange(n) % 2 == 1, f32(1.0), f32(2.0)).astype(f32)
    specs = [(np.full(n, 0.125, f32), np.zeros(n, f32), 0, 0, 0), (two, striped, 1, 1, 0), (np.ones(n, f32), two, 2, 3, 1),
             (_values(rng, n), np.full(n, -1e-3, f32), 3, 3, 0)]
    unset = -2 ** 31
    ssd.set_option("hist_scheme", unset if scheme is None else scheme)
    try:
        c, s, _ = _run_and_check(ssd, cuda, limits_dev, specs, "contention scheme %r" % (scheme,))
    finally:
        ssd.set_option("hist_scheme", unset)
    assert c[0, 0].max() == n and c[0, 1].max() == n and np.count_nonzero(c[1, 0]) == 2 and np.count_nonzero(c[1, 1]) == 2
    assert (c.sum(axis=2) == n).all()


def test_forty_tensors_with_an_empty_one_and_the_norms_cross_check(ssd, cuda, limits_dev):
    rng = np.random.default_rng(1)
    sizes = [int(v) for v in rng.integers(1, 9000, 41)]
    sizes[20] = 0
    specs = []
    for i, n in enumerate(sizes):
        g = None if i % 5 == 4 else _values(rng, n)
        specs.append((_values(rng, n), g, i % 4, (i // 4) % 4, (i // 2) & 1))
    c, s, (host, devrows, _arena) = _run_and_check(ssd, cuda, limits_dev, specs, "forty")
    assert c[20].sum() == 0 and s["num"][20].tolist() == [0, 0] and s["sum"][20].tolist() == [0.0, 0.0]
    assert s["min"][20].tolist() == [np.inf, np.inf] and s["max"][20].tolist() == [-np.inf, -np.inf]
    # sum_squares of every w plane, and of the gradient plane where decay == 0, has ssd_train_norms' bits
    T = len(specs)
    sums = cuda.empty((T, 2), dtype=cuda.float64, device="cuda")
    bad = cuda.empty((T, 2), dtype=cuda.int64, device="cuda")
    ssd.train_calls.train_norms(host, devrows, sums, bad)
    sums = sums.cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(s["sum_squares"][:, 0]).view(np.int64), sums[:, 0].copy().view(np.int64))
    plain = np.array([sp[4] == 0 for sp in specs])
    assert plain.sum() >= 15
    assert np.array_equal(np.ascontiguousarray(s["sum_squares"][plain, 1]).view(np.int64), sums[plain, 1].copy().view(np.int64))
    decaying = ~plain & np.array([sp[1] is not None and len(sp[0]) > 0 for sp in specs])
    assert (s["sum_squares"][decaying, 1] != sums[decaying, 1]).all()


def test_refusals_leave_the_outputs_untouched(ssd, cuda, limits_dev):
    rng = np.random.default_rng(4)
    _arena, host, devrows, blocks, _want = _table(cuda, [(_values(rng, 5000), _values(rng, 5000), 0, 0, 1)])
    L, NB = ssd.lib(), ref.NB
    counts = cuda.full((1, 2, NB), 77, dtype=cuda.int64, device="cuda")
    stats = cuda.full((1, 2, 40), 0x33, dtype=cuda.uint8, device="cuda")
    ws = cuda.full((64 * blocks,), 0x44, dtype=cuda.uint8, device="cuda")
    stream = cuda.cuda.current_stream().cuda_stream
    p = ctypes.c_void_p

    def call(rows=host.data_ptr(), T=1, wd=1e-4, lim=limits_dev.data_ptr(), c=counts.data_ptr(), s=stats.data_ptr(), w=ws.data_ptr(),
             nbytes=ws.numel()):
        return L.ssd_train_histograms(p(rows), p(devrows.data_ptr()), T, wd, p(lim), p(c), p(s), p(w), nbytes, p(stream))
    for kw in ({"T": 0}, {"wd": float("nan")}, {"wd": float("-inf")}, {"lim": 0}, {"c": 0}, {"s": 0}, {"w": 0},
               {"lim": limits_dev.data_ptr() + 4}, {"c": counts.data_ptr() + 4}, {"s": stats.data_ptr() + 4}, {"w": ws.data_ptr() + 8},
               {"nbytes": ws.numel() - 1}):
        assert call(**kw) == -1, kw
        assert L.ssd_last_error().decode().startswith("ssd_train_histograms:"), kw
    cuda.cuda.synchronize()
    assert bool((counts == 77).all()) and bool((stats == 0x33).all()) and bool((ws == 0x44).all())
    assert call() == 0
    cuda.cuda.synchronize()
    assert int(counts.sum()) == 10000


def test_trainstep_histograms_after_a_real_backward_of_the_head(ssd, cuda):
    rng = np.random.default_rng(3)
    W = ssd.synthetic_weights(TINY_PARAMS, seed=5, logits_bias=-4.0)
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-2}
    m = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").train()
    ts = ssd.TrainStep(m.named_variables(), cfg, m.statistics(), layout="tf", params=TINY_PARAMS)
    feats = [_dev(cuda, rng.normal(0, 1, (2, s, s, 256))) for s in (16, 8, 4, 2, 1)]
    anchors, boxes, labels, num = href.groundtruth(ssd, 2, 9)
    eb, cp = m(feats)
    out = ssd.differentiable_loss(cp, eb, _dev(cuda, anchors), {"boxes": boxes, "labels": labels, "num_boxes": num},
                                  {"gamma": 2.0, "alpha": 0.25})
    (out["localization_loss"] + out["classification_loss"]).backward()
    ts.parameters[ts.names[3]].grad = None                           # a NULL gradient row
    assert ts._hist_ring is None and ts._hist_limits is None         # made by the first call
    rings = [id(s["host"]) for s in ts._ring.slots] + [id(s["host"]) for s in (ts._norms_ring.slots if ts._norms_ring else [])]
    counts, stats = ts.histograms()
    T, NB = len(ts.names), ref.NB
    assert tuple(counts.shape) == (T, 2, NB) and counts.dtype == cuda.int64 and tuple(stats.shape) == (T, 2, 40) and stats.dtype == cuda.uint8
    limits = ts._hist_limits
    again = ts.histograms()
    assert ts._hist_limits is limits                                 # uploaded once
    assert not set(id(s["host"]) for s in ts._hist_ring.slots) & set(rings)
    c, s = counts.cpu().numpy(), _host_stats(stats)
    assert np.array_equal(again[0].cpu().numpy(), c) and _host_stats(again[1]).tobytes() == s.tobytes()
    want = []
    for name in ts.names:
        p = ts.parameters[name]
        want.append((p.detach().cpu().numpy().reshape(-1), None if p.grad is None else p.grad.cpu().numpy().reshape(-1),
                     (p.data_ptr() // 4) % 4, 1 if ssd.train_step.decays(name) else 0))
    want_c, want_s = ref.table_histograms(want, f32(cfg["weight_decay"]))
    _compare("TrainStep", c, s, want_c, want_s)
    assert s["num"][3, 1] == 0 and c[3, 1].sum() == 0 and not s["bad"].any()
    sums, _bad = ts.norms()
    assert np.array_equal(np.ascontiguousarray(s["sum_squares"][:, 0]).view(np.int64), sums.cpu().numpy()[:, 0].copy().view(np.int64))
    pinned = [slot["host"].data_ptr() for ring in (ts._ring, ts._norms_ring, ts._hist_ring) for slot in ring.slots]
    assert len(set(pinned)) == 3 * ts.RING                           # the three rings are pairwise distinct pinned buffers
    # refused under stream capture, for norms()' reason; the capture around it stays usable
    x = cuda.zeros(8, device="cuda")
    cuda.cuda.synchronize()
    graph = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            ts.histograms()
    graph.replay()
    cuda.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [1.0] * 8
