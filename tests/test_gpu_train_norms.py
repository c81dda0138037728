"""ssd_train_norms on the GPU against its numpy restatement (helpers/train_norms_ref.py), bit for bit: tensor sizes around the block
size at every offset of w inside its 16-byte group, gradients of w's alignment class, of another one and NULL, a table with an empty
tensor in the middle, values whose sum depends on the order of the additions, NaN and infinities on the ends of a tensor and across a
block boundary; outputs and workspace pre-filled with NaN bytes behind guard words; TrainStep.norms() after a real backward of the head; and
norms() and histograms() past one turn of their pinned rings while the stream is still busy."""
import numpy as np
import pytest

from helpers import head_train_ref as href
from helpers import train_norms_ref as ref
from helpers.head_train_gpu import dev as _dev
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
COUNTS = (1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5)
GUARD = 0x5A
NAN_BYTE = 0xFF                          # float64 / float32 of 0xFF bytes is a NaN, int64 is -1


def _values(rng, n):
    """Random signs and mantissas over +-40 binades: the order of the additions shows in the last bits of the sum."""
    return (rng.normal(0, 1, n) * np.exp2(rng.integers(-40, 41, n))).astype(f32)


class _Arena:
    """Tensors at chosen float offsets from a 16-byte boundary inside one device buffer."""

    def __init__(self, cuda, floats):
        self.cuda = cuda
        self.buf = cuda.zeros(floats, dtype=cuda.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.at = 0

    def put(self, host, offset):
        """A device view holding `host` whose first element sits `offset` floats (0..3) after a 16-byte boundary."""
        start = (self.at + 3) // 4 * 4 + offset
        self.at = start + max(len(host), 1)
        view = self.buf[start:start + len(host)]
        if len(host):
            view.copy_(self.cuda.from_numpy(host))
        assert (self.buf.data_ptr() + 4 * start) % 16 == 4 * offset
        return view, self.buf.data_ptr() + 4 * start


def _table(ssd, cuda, specs):
    """specs: (w host array, grad host array or None, w offset, grad offset) per row -> the device tensors, the rows (host uint8
    tensor, device copy), and the restatement's input."""
    from ssd_amd import train_step
    arena = _Arena(cuda, sum(len(w) + 8 + (len(g) + 8 if g is not None else 0) for w, g, _a, _b in specs) + 16)
    rows = np.zeros(len(specs), train_step.TENSOR_DTYPE)
    held, want = [], []
    for t, (w, g, wo, go) in enumerate(specs):
        wt, wp = arena.put(w, wo)
        gt, gp = arena.put(g, go) if g is not None else (None, 0)
        rows[t]["w"], rows[t]["grad"], rows[t]["count"] = wp, gp, len(w)
        rows[t]["m"] = rows[t]["v"] = rows[t]["ema"] = wp              # validated, never dereferenced
        rows[t]["decay"] = t & 1
        held.append((wt, gt))
        want.append((w, g, wo))
    rows["first_block"], blocks = train_step.block_starts(rows["w"], rows["count"])
    host = cuda.from_numpy(rows.view(np.uint8).copy())
    return arena, held, host, host.cuda(), blocks, want


def _guarded(cuda, shape, dtype, guard_rows=1):
    """A tensor of `shape` pre-filled with NaN bytes between guard rows -> (the whole buffer as bytes, the inner view)."""
    full = cuda.empty((shape[0] + 2 * guard_rows,) + tuple(shape[1:]), dtype=dtype, device="cuda")
    raw = full.view(cuda.uint8)
    raw.fill_(GUARD)
    inner = full[guard_rows:guard_rows + shape[0]]
    inner.view(cuda.uint8).fill_(NAN_BYTE)
    return raw, inner


def _run_and_check(ssd, cuda, specs, tag):
    arena, held, host, devrows, blocks, want = _table(ssd, cuda, specs)
    calls = ssd.train_calls
    T = len(specs)
    need = calls.train_norms_workspace_bytes(host)
    assert need == 32 * blocks
    sraw, sums = _guarded(cuda, (T, 2), cuda.float64)
    braw, bad = _guarded(cuda, (T, 2), cuda.int64)
    wraw = cuda.full((need + 32,), GUARD, dtype=cuda.uint8, device="cuda")
    ws = wraw[16:16 + need]
    ws.fill_(NAN_BYTE)
    assert ws.data_ptr() % 16 == 0
    before = arena.buf.clone()
    calls.train_norms(host, devrows, sums, bad, workspace=ws)
    s1, b1 = sums.cpu().numpy().copy(), bad.cpu().numpy().copy()
    sums.view(cuda.uint8).fill_(NAN_BYTE)
    bad.view(cuda.uint8).fill_(NAN_BYTE)
    calls.train_norms(host, devrows, sums, bad, workspace=ws)
    s2, b2 = sums.cpu().numpy(), bad.cpu().numpy()
    want_s, want_b = ref.table_norms(want)
    assert np.array_equal(b1, want_b), (tag, np.nonzero(b1 != want_b))
    wrong = np.nonzero(s1.view(np.int64) != want_s.view(np.int64))
    assert len(wrong[0]) == 0, (tag, wrong, s1[wrong], want_s[wrong])
    assert np.array_equal(s1.view(np.int64), s2.view(np.int64)) and np.array_equal(b1, b2), tag     # two calls, the same bits
    assert cuda.equal(arena.buf.view(cuda.int32), before.view(cuda.int32)), tag                     # w and grad keep their bits
    for raw, inner_bytes in ((sraw, T * 16), (braw, T * 16)):
        r = raw.reshape(-1).cpu().numpy()
        assert (r[:16] == GUARD).all() and (r[16 + inner_bytes:] == GUARD).all(), tag
    r = wraw.cpu().numpy()
    assert (r[:16] == GUARD).all() and (r[16 + need:] == GUARD).all(), tag
    return s1, b1


def _sweep_specs(rng):
    """Every count at every w offset, with a gradient of w's class, of another class, and NULL."""
    specs = []
    for n in COUNTS:
        for wo in range(4):
            specs.append((_values(rng, n), _values(rng, n), wo, wo))
            specs.append((_values(rng, n), _values(rng, n), wo, (wo + 1 + (n + wo) % 3) % 4))
            specs.append((_values(rng, n), None, wo, 0))
    return specs


def test_sizes_offsets_and_gradient_classes_in_one_table(ssd, cuda):
    specs = _sweep_specs(np.random.default_rng(0))
    assert len(specs) == 84 and all(g is None or go != wo or i % 3 == 0 for i, (_w, g, wo, go) in enumerate(specs))
    s, b = _run_and_check(ssd, cuda, specs, "sweep")
    assert not b.any() and (s[:, 0] > 0).all() and (s[2::3, 1] == 0).all() and (s[0::3, 1] > 0).all() and (s[1::3, 1] > 0).all()


@pytest.mark.parametrize("n,wo,go", [(1, 3, 3), (4097, 1, 1), (4097, 2, 0), (3 * 4096 + 5, 0, None), (4096, 3, 2)])
def test_a_table_of_one_tensor(ssd, cuda, n, wo, go):
    rng = np.random.default_rng(n + wo)
    _run_and_check(ssd, cuda, [(_values(rng, n), _values(rng, n) if go is not None else None, wo, go or 0)], "T = 1")


def test_forty_tensors_with_an_empty_one_in_the_middle(ssd, cuda):
    rng = np.random.default_rng(1)
    sizes = [int(v) for v in rng.integers(1, 9000, 41)]
    sizes[20] = 0
    specs = []
    for i, n in enumerate(sizes):
        g = None if i % 5 == 4 else _values(rng, n)
        specs.append((_values(rng, n), g, i % 4, (i // 4) % 4))
    s, b = _run_and_check(ssd, cuda, specs, "forty")
    assert s[20].tolist() == [0.0, 0.0] and b[20].tolist() == [0, 0]


def test_non_finite_elements_on_the_ends_and_across_a_block_boundary(ssd, cuda):
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
        specs.append((w, g, wo, go))
        planted.append([4, 5])
    w = _values(rng, 3)
    w[:] = [np.nan, np.inf, -np.inf]                                 # nothing finite: sum +0.0
    specs.append((w, None, 1, 0))
    planted.append([3, 0])
    s, b = _run_and_check(ssd, cuda, specs, "non-finite")
    assert b.tolist() == planted and np.isfinite(s).all() and s[4].tolist() == [0.0, 0.0]


def test_trainstep_norms_after_a_real_backward_of_the_head(ssd, cuda):
    """Every row against the restatement on the read-back tensors; regularization_loss against evaluation.regularization_loss of
    the same variables: the double sums differ only in their order (about 1e-9 relative at most), so the float32 results are equal
    or neighbours."""
    from ssd_amd import evaluation
    rng = np.random.default_rng(3)
    W = ssd.synthetic_weights(TINY_PARAMS, seed=5, logits_bias=-4.0)
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
    m = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda").train()
    ts = ssd.TrainStep(m.named_variables(), cfg, m.statistics(), layout="tf", params=TINY_PARAMS)
    feats = [_dev(cuda, rng.normal(0, 1, (2, s, s, 256))) for s in (16, 8, 4, 2, 1)]
    anchors, boxes, labels, num = href.groundtruth(ssd, 2, 9)
    eb, cp = m(feats)
    out = ssd.differentiable_loss(cp, eb, _dev(cuda, anchors), {"boxes": boxes, "labels": labels, "num_boxes": num},
                                  {"gamma": 2.0, "alpha": 0.25})
    (out["localization_loss"] + out["classification_loss"]).backward()
    skipped = ts.names[3]
    ts.parameters[skipped].grad = None                               # a NULL gradient row
    sums, bad = ts.norms()
    assert tuple(sums.shape) == (len(ts.names), 2) == tuple(bad.shape) and sums.dtype == cuda.float64 and bad.dtype == cuda.int64
    again = ts.norms()
    sums, bad = sums.cpu().numpy(), bad.cpu().numpy()
    assert np.array_equal(again[0].cpu().numpy().view(np.int64), sums.view(np.int64)) and not bad.any()
    want = []
    for name in ts.names:
        p = ts.parameters[name]
        want.append((p.detach().cpu().numpy().reshape(-1), None if p.grad is None else p.grad.cpu().numpy().reshape(-1),
                     (p.data_ptr() // 4) % 4))
    want_s, want_b = ref.table_norms(want)
    assert np.array_equal(sums.view(np.int64), want_s.view(np.int64)) and np.array_equal(bad, want_b)
    assert sums[3, 1] == 0 and (np.delete(sums[:, 1], 3) > 0).sum() >= len(ts.names) - 20      # p6 / p7 batch norms may be silent
    got = ts.regularization_loss(sums)
    host = {n: ts.parameters[n].detach().cpu().numpy() for n in ts.names}
    ref_loss = evaluation.regularization_loss(host, cfg["weight_decay"])
    print("regularization_loss: norms %r, evaluation %r" % (float(got), float(ref_loss)))
    assert got.dtype == np.float32 and got > 0
    assert got == ref_loss or got in (np.nextafter(ref_loss, f32(np.inf)), np.nextafter(ref_loss, f32(-np.inf)))
    # refused under stream capture, for step()'s reason; the capture around it stays usable
    x = cuda.zeros(8, device="cuda")
    cuda.cuda.synchronize()
    graph = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            ts.norms()
    graph.replay()
    cuda.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [1.0] * 8


def test_norms_and_histograms_reuse_every_pinned_slot_while_the_stream_is_busy(ssd, cuda):
    """RING + 2 calls of norms() and of histograms() back to back, each on a gradient set of its own (all allocated before, all alive:
    every address is distinct), enqueued behind work that keeps the stream busy, so that the uploads of the first calls have not run
    when their pinned slots come round again.  One synchronise at the end; call k must report call k's gradients bit for bit (the
    restatements of helpers/train_norms_ref.py and helpers/histogram_ref.py).  A slot rewritten before its upload ran shows as call k
    reporting the gradients of call k + RING."""
    from helpers import histogram_ref
    from test_gpu_train_histograms import _compare, _host_stats
    rng = np.random.default_rng(11)
    sizes = {"a/weights": 5, "b/beta": 64, "c/kernel": 1031}
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 0.5}
    P = {n: cuda.from_numpy(_values(rng, c)).cuda().requires_grad_() for n, c in sizes.items()}
    ts = ssd.TrainStep(P, cfg, layout="tf")
    calls = ts.RING + 2
    host = [[_values(rng, c) for c in sizes.values()] for _ in range(calls)]
    grads = [[cuda.from_numpy(g).cuda() for g in gs] for gs in host]
    assert len({g.data_ptr() for gs in grads for g in gs}) == calls * len(sizes)
    busy = cuda.zeros(1 << 27, device="cuda")
    cuda.cuda.synchronize()
    for _ in range(40):
        busy.add_(1.0)                                               # 1 GiB of traffic each: the stream stays behind the host
    got = []
    for gs in grads:
        for p, g in zip(P.values(), gs):
            p.grad = g
        got.append((ts.norms(), ts.histograms()))
    cuda.cuda.synchronize()
    w = [(p.detach().cpu().numpy(), (p.data_ptr() // 4) % 4, 1 if ssd.train_step.decays(n) else 0) for n, p in P.items()]
    assert [d for _w, _o, d in w] == [1, 0, 1]
    for k, ((sums, bad), (counts, stats)) in enumerate(got):
        want_s, want_b = ref.table_norms([(x, g, wo) for (x, wo, _d), g in zip(w, host[k])])
        assert np.array_equal(sums.cpu().numpy().view(np.int64), want_s.view(np.int64)) and np.array_equal(bad.cpu().numpy(), want_b), k
        want_c, want_st = histogram_ref.table_histograms([(x, g, wo, d) for (x, wo, d), g in zip(w, host[k])], f32(cfg["weight_decay"]))
        _compare("call %d" % k, counts.cpu().numpy(), _host_stats(stats), want_c, want_st)
    assert len({sums.cpu().numpy().tobytes() for (sums, _b), _h in got}) == calls      # the calls differ: none stood in for another
