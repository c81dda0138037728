"""The TRAIN update on the GPU: csrc/update.hip through the raw entry point, bit for bit against the numpy float32 restatement
(tests/helpers/train_update_ref.py); TrainStep on top of it; checkpoints out and back in; thirty steps of a small torch head."""
import ctypes

import numpy as np
import pytest

from helpers import train_update_ref as ref

pytestmark = pytest.mark.gpu

CFG = {"initial_learning_rate": 1e-3, "num_steps": 1000, "weight_decay": 5e-5}
MOBILENET = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
SHUFFLENET = {"backbone": "shufflenet", "depth_multiplier": 1.0, "num_classes": 80}
GUARD = 8                                    # guard words on either side of every tensor
SENTINEL = np.uint32(0x7FC0DEAD)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gradient(rng, n):
    """Magnitudes 1e-8 .. 1e2, both signs, exact zeros and denormals."""
    g = (10.0 ** rng.uniform(-8, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    k = rng.random(n) < 0.02
    g[k] = (rng.uniform(-1, 1, int(k.sum())) * 1e-39).astype(np.float32)
    return g


def _layout(counts, offsets):
    """Element offsets of every tensor inside a flat buffer: GUARD words before and after each, tensor i starting `offsets[i]`
    elements past a 16-byte boundary.  -> (starts, total)."""
    starts, cursor = [], 0
    for n, off in zip(counts, offsets):
        s = (cursor + GUARD + 3) // 4 * 4 + off
        starts.append(s)
        cursor = s + n + GUARD
    return starts, (cursor + 3) // 4 * 4


class _Flat:
    """One flat device buffer holding every tensor of one kind (w, m, v, ema or a step's gradients) between guard words."""

    def __init__(self, torch, arrays, counts, offsets):
        self.starts, total = _layout(counts, offsets)
        host = np.full(total, SENTINEL, np.uint32)
        self.mask = np.ones(total, bool)                       # True: a guard word
        for a, s, n in zip(arrays, self.starts, counts):
            self.mask[s:s + n] = False
            if a is not None:
                host[s:s + n] = _bits(a)
        self.host = host
        self.dev = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.starts[i]

    def read(self, counts):
        out = self.dev.cpu().numpy().view(np.uint32)
        assert np.array_equal(out[self.mask], self.host[self.mask]), "a guard word was overwritten"
        return [out[s:s + n].view(np.float32).copy() for s, n in zip(self.starts, counts)]


def _run_raw(ssd, torch, cfg, state, grads_per_step, decay, offsets, first_t=1):
    """state: per tensor [w, m, v, ema] float32 arrays; offsets: per tensor a dict kind -> element offset past a 16-byte boundary.
    Runs ssd_train_update once per step and returns the per-tensor [w, m, v, ema] read back; guards are checked on every buffer,
    gradients must come back untouched."""
    from ssd_amd import train_step, _lib
    L = ssd.lib()
    T = len(state)
    counts = [len(s[0]) for s in state]
    bufs = {k: _Flat(torch, [s[j] for s in state], counts, [o[k] for o in offsets]) for j, k in enumerate(("w", "m", "v", "ema"))}
    rows = np.zeros(T, train_step.TENSOR_DTYPE)
    for k in ("w", "m", "v", "ema"):
        rows[k] = [bufs[k].ptr(i) for i in range(T)]
    rows["count"] = counts
    rows["decay"] = [int(d) for d in decay]
    rows["first_block"], _total = train_step.block_starts(rows["w"], rows["count"])
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    for k, grads in enumerate(grads_per_step):
        gb = _Flat(torch, grads, counts, [o["grad"] for o in offsets])
        r = rows.copy()
        r["grad"] = [gb.ptr(i) if g is not None else 0 for i, g in enumerate(grads)]
        dev = torch.from_numpy(r.view(np.uint8)).cuda()
        sc = train_step.step_scalars(cfg, first_t + k)
        rc = L.ssd_train_update(r.ctypes.data_as(ctypes.c_void_p), dev.data_ptr(), T, ctypes.byref(sc), stream)
        assert rc == 0, L.ssd_last_error()
        keep.append((gb, r, dev))
    torch.cuda.synchronize()
    for gb, _r, _dev in keep:
        assert np.array_equal(gb.dev.cpu().numpy().view(np.uint32), gb.host), "a gradient buffer was written"
    got = [bufs[k].read(counts) for k in ("w", "m", "v", "ema")]
    return [[got[j][i] for j in range(4)] for i in range(T)]


def _case(rng, counts, steps, null_share=0.1, scale=None):
    state = []
    for i, n in enumerate(counts):
        w = rng.normal(0, 1.0 if scale is None else scale[i], n).astype(np.float32)
        state.append([w, np.zeros(n, np.float32), np.zeros(n, np.float32), w.copy()])
    grads = [[None if rng.random() < null_share else _gradient(rng, n) for n in counts] for _ in range(steps)]
    return state, grads


def _assert_same_bits(got, want, names=None):
    for i, (g, w) in enumerate(zip(got, want)):
        for j, kind in enumerate(("w", "m", "v", "ema")):
            same = np.array_equal(_bits(g[j]), _bits(w[j]))
            if not same:
                bad = np.nonzero(_bits(g[j]) != _bits(w[j]))[0]
                raise AssertionError("tensor %s (%d elements): %s differs at %d elements, first %d: got %r want %r"
                                     % (names[i] if names else i, len(w[j]), kind, len(bad), bad[0], g[j][bad[0]], w[j][bad[0]]))


def _same_offsets(T, off):
    return [dict.fromkeys(("w", "grad", "m", "v", "ema"), off(i) if callable(off) else off) for i in range(T)]


@pytest.mark.parametrize("views", [False, True], ids=["aligned", "views_at_1_2_3"])
@pytest.mark.parametrize("params", [MOBILENET, SHUFFLENET], ids=["mobilenet", "shufflenet"])
def test_full_trainable_set_is_bit_identical_to_the_helper(ssd, cuda, params, views):
    """Every trainable tensor of the architecture in one launch, 3 consecutive steps, about one tensor in ten without a gradient;
    `views`: tensor i starts 1 + i % 3 elements past a 16-byte boundary in every buffer (4-byte-aligned bases)."""
    from ssd_amd import train_step
    W = ssd.synthetic_weights(params, seed=11)
    names = train_step.trainable_names(params)
    rng = np.random.default_rng(12)
    counts = [W[n].size for n in names]
    state, grads = _case(rng, counts, 3)
    for s, n in zip(state, names):
        s[0][:] = W[n].reshape(-1)
        s[3][:] = s[0]
    decay = [train_step.decays(n) for n in names]
    assert sum(decay) == (32 if params is MOBILENET else 55)
    assert any(g is None for gs in grads for g in gs)
    want = [[a.copy() for a in s] for s in state]
    ref.run(CFG, want, grads, [ref.decays(n) for n in names])
    got = _run_raw(ssd, cuda, CFG, state, grads, decay, _same_offsets(len(names), (lambda i: 1 + i % 3) if views else 0))
    _assert_same_bits(got, want, names)


@pytest.mark.parametrize("offset", [0, 1, 2, 3, "mixed"])
def test_small_and_odd_counts_at_every_alignment(ssd, cuda, offset):
    """Counts around the quad and the block size at every start inside a 16-byte group; "mixed": the five buffers of a tensor
    start at different offsets, which takes the element-by-element path."""
    counts = [1, 3, 5, 1023, 1025, 2, 4, 4093, 4094, 4095, 4096, 4097, 8191, 8193, 12291, 7]
    rng = np.random.default_rng(20 + (offset if offset != "mixed" else 9))
    state, grads = _case(rng, counts, 3, null_share=0.15)
    decay = [i % 2 == 0 for i in range(len(counts))]
    want = [[a.copy() for a in s] for s in state]
    ref.run(CFG, want, grads, decay)
    if offset == "mixed":
        offsets = [{"w": i % 4, "grad": (i + 1) % 4, "m": (i // 2) % 4, "v": 3 - i % 4, "ema": (i + 2) % 4} for i in range(len(counts))]
        offsets[3] = {"w": 2, "m": 2, "v": 2, "ema": 2, "grad": 1}              # only the gradient is off
    else:
        offsets = _same_offsets(len(counts), offset)
    _assert_same_bits(_run_raw(ssd, cuda, CFG, state, grads, decay, offsets), want)


def test_two_runs_give_the_same_bits(ssd, cuda):
    counts = [70000, 513, 4096, 9, 30001]
    state, grads = _case(np.random.default_rng(30), counts, 3)
    decay = [True, False, True, False, True]
    a = _run_raw(ssd, cuda, CFG, state, grads, decay, _same_offsets(5, 0))
    b = _run_raw(ssd, cuda, CFG, state, grads, decay, _same_offsets(5, 0))
    _assert_same_bits(a, b)


def test_captured_launch_replays_the_same_update(ssd, cuda):
    """The raw entry point only enqueues one kernel: it may be captured (one node, no branches); two replays are two updates with
    the captured scalars."""
    from ssd_amd import train_step
    L = ssd.lib()
    n = 10000
    rng = np.random.default_rng(31)
    w0 = rng.normal(0, 1, n).astype(np.float32)
    g = _gradient(rng, n)
    dev = {k: cuda.from_numpy(a.copy()).cuda() for k, a in (("w", w0), ("grad", g), ("m", np.zeros(n, np.float32)),
                                                            ("v", np.zeros(n, np.float32)), ("ema", w0))}
    rows = np.zeros(1, train_step.TENSOR_DTYPE)
    for k in dev:
        rows[k] = dev[k].data_ptr()
    rows["count"], rows["decay"] = n, 1
    table = cuda.from_numpy(rows.view(np.uint8)).cuda()
    sc = train_step.step_scalars(CFG, 1)
    cuda.cuda.synchronize()
    graph = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(graph):
        rc = L.ssd_train_update(rows.ctypes.data_as(ctypes.c_void_p), table.data_ptr(), 1, ctypes.byref(sc),
                                cuda.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ssd_last_error()
    cuda.cuda.synchronize()
    assert np.array_equal(dev["w"].cpu().numpy(), w0)                         # capturing ran nothing
    graph.replay()
    graph.replay()
    cuda.cuda.synchronize()
    want = [w0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), w0.copy()]
    for _ in range(2):
        ref.update(want[0], g, want[1], want[2], want[3], True, ref.scalars(CFG, 1))
    _assert_same_bits([[dev[k].cpu().numpy() for k in ("w", "m", "v", "ema")]], [want])


# ----------------------------------------------------------------------------- TrainStep
SMALL = [("fpn/p3/kernel", (16, 12, 3, 3)), ("MobilenetV1/Conv2d_1_depthwise/depthwise_weights", (24, 1, 3, 3)),
         ("MobilenetV1/Conv2d_1_depthwise/BatchNorm/gamma", (24,)), ("MobilenetV1/Conv2d_1_depthwise/BatchNorm/beta", (24,)),
         ("MobilenetV1/Conv2d_1_pointwise/weights", (40, 24, 1, 1)), ("box_net/encoded_boxes/kernel", (24, 129, 3, 3)),
         ("box_net/encoded_boxes/bias", (24,)), ("class_net/logits/kernel", (37, 64, 3, 3)), ("class_net/logits/bias", (1,))]
SMALL_STATS = [("MobilenetV1/Conv2d_1_depthwise/BatchNorm/moving_mean", (24,)),
               ("MobilenetV1/Conv2d_1_depthwise/BatchNorm/moving_variance", (24,))]


def _small_model(torch, seed):
    rng = np.random.default_rng(seed)
    P = {n: torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).cuda().requires_grad_(True) for n, s in SMALL}
    S = {n: torch.from_numpy(rng.uniform(0.5, 1.5, s).astype(np.float32)).cuda() for n, s in SMALL_STATS}
    return P, S


def _small_grads(steps, seed):
    rng = np.random.default_rng(seed)
    return [[None if (k + i) % 5 == 4 else _gradient(rng, int(np.prod(s))).reshape(s) for i, (_n, s) in enumerate(SMALL)]
            for k in range(steps)]


def _drive(torch, ts, P, grads):
    for gs in grads:
        for (n, _s), g in zip(SMALL, gs):
            P[n].grad = None if g is None else torch.from_numpy(g).cuda()        # a fresh allocation every step, as autograd makes
        ts.step()


def _read(ts, P):
    return [[P[n].detach().cpu().numpy().reshape(-1)] + [x.cpu().numpy().reshape(-1) for x in ts.slots(n)] +
            [ts.ema(n).cpu().numpy().reshape(-1)] for n, _s in SMALL]


def test_train_step_equals_the_raw_entry_point(ssd, cuda):
    P, S = _small_model(cuda, 40)
    start = [[P[n].detach().cpu().numpy().reshape(-1).copy() for _ in range(1)] for n, _s in SMALL]
    ts = ssd.TrainStep(P, CFG, statistics=S)
    assert ts.global_step == 0
    for n, _s in SMALL:
        m, v = ts.slots(n)
        assert m.shape == P[n].shape and not m.any() and not v.any() and cuda.equal(ts.ema(n), P[n].detach())
    grads = _small_grads(6, 41)                        # 6 > RING: every pinned slot is reused
    _drive(cuda, ts, P, grads)
    assert ts.global_step == 6
    got = _read(ts, P)
    state = [[w[0], np.zeros_like(w[0]), np.zeros_like(w[0]), w[0].copy()] for w in start]
    flat = [[None if g is None else g.reshape(-1) for g in gs] for gs in grads]
    decay = [ref.decays(n) for n, _s in SMALL]
    assert decay == [True, False, False, False, True, True, False, True, False]
    raw = _run_raw(ssd, cuda, CFG, state, flat, decay, _same_offsets(len(SMALL), 0))
    _assert_same_bits(got, raw, [n for n, _ in SMALL])
    want = [[a.copy() for a in s] for s in state]
    ref.run(CFG, want, flat, decay)
    _assert_same_bits(got, want, [n for n, _ in SMALL])


def test_train_step_refuses_what_it_cannot_update(ssd, cuda):
    P, S = _small_model(cuda, 42)
    with pytest.raises(ValueError, match="fpn/p3/kernel"):
        ssd.TrainStep(P, CFG, params=MOBILENET)                                  # a known name with another shape
    with pytest.raises(KeyError, match="no/such/weights"):
        ssd.TrainStep({"no/such/weights": P["fpn/p3/kernel"]}, CFG, params=MOBILENET)
    with pytest.raises(KeyError, match="moving_mean"):                           # a statistic is not trainable
        ssd.TrainStep({SMALL_STATS[0][0]: P["box_net/encoded_boxes/bias"]}, CFG, params=MOBILENET)
    with pytest.raises(TypeError):
        ssd.TrainStep({"a/weights": cuda.zeros(4, dtype=cuda.float64, device="cuda", requires_grad=True)}, CFG)
    with pytest.raises(ValueError):
        ssd.TrainStep({"a/weights": cuda.zeros(4, requires_grad=True)}, CFG)       # a CPU tensor
    base = cuda.zeros(16, device="cuda")
    with pytest.raises(ValueError, match="share storage"):
        ssd.TrainStep({"a/weights": base[:8].detach().requires_grad_(True), "b/weights": base[4:12].detach().requires_grad_(True)}, CFG)
    with pytest.raises(KeyError):
        ssd.TrainStep(P, CFG, statistics={"fpn/p3/kernel/not_a_statistic": S[SMALL_STATS[0][0]]})
    with pytest.raises(KeyError):
        ssd.TrainStep(P, {"num_steps": 10, "weight_decay": 0.0})


def test_step_is_refused_under_graph_capture_and_the_capture_survives(ssd, cuda):
    """step() reads the gradients' addresses and forms the step's scalars on the host, so a captured step would replay stale
    values: it raises before it enqueues anything, and the capture around it stays usable."""
    P, S = _small_model(cuda, 43)
    ts = ssd.TrainStep(P, CFG, statistics=S)
    grads = _small_grads(1, 44)
    for (n, _s), g in zip(SMALL, grads[0]):
        P[n].grad = None if g is None else cuda.from_numpy(g).cuda()
    x = cuda.zeros(8, device="cuda")
    cuda.cuda.synchronize()
    graph = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            ts.step()
    assert ts.global_step == 0
    graph.replay()
    cuda.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [1.0] * 8
    before = _read(ts, P)
    assert all(not a[1].any() and np.array_equal(a[0], a[3]) for a in before)      # nothing ran
    ts.step()                                                                      # and outside the capture it runs
    want = [[a.copy() for a in s] for s in before]
    ref.run(CFG, want, [[None if g is None else g.reshape(-1) for g in grads[0]]], [ref.decays(n) for n, _s in SMALL])
    _assert_same_bits(_read(ts, P), want)


@pytest.mark.parametrize("layout", ["torch", "tf"])
def test_save_restore_continues_bit_identically(ssd, cuda, tmp_path, layout):
    from ssd_amd import train_step
    grads = _small_grads(5, 51)
    P, S = _small_model(cuda, 50)
    ts = ssd.TrainStep(P, CFG, statistics=S, layout=layout)
    _drive(cuda, ts, P, grads)
    want = _read(ts, P)

    P1, S1 = _small_model(cuda, 50)
    t1 = ssd.TrainStep(P1, CFG, statistics=S1, layout=layout)
    _drive(cuda, t1, P1, grads[:3])
    prefix = t1.save(str(tmp_path / "run"))
    assert prefix.endswith("model.ckpt-3") and ssd.resolve_checkpoint(str(tmp_path / "run")) == prefix
    stored = ssd.read_checkpoint(prefix, verify=True)
    assert stored["global_step"].dtype == np.int64 and stored["global_step"].shape == () and int(stored["global_step"]) == 3
    assert stored["optimizer/beta1_power"] == np.float32(0.9 ** 4) and stored["optimizer/beta2_power"] == np.float32(0.999 ** 4)
    assert len(stored) == 4 * len(SMALL) + len(SMALL_STATS) + 3
    for n, s in SMALL:
        tf_shape = s if layout == "tf" or len(s) != 4 else train_step.to_tf_layout(n, np.zeros(s, np.float32)).shape
        for key, t in ((n, P1[n]), (n + "/ExponentialMovingAverage", t1.ema(n)), ("optimizer/%s/Adam" % n, t1.slots(n)[0]),
                       ("optimizer/%s/Adam_1" % n, t1.slots(n)[1])):
            a = t.detach().cpu().numpy()
            assert stored[key].shape == tuple(tf_shape), key
            assert np.array_equal(_bits(stored[key]), _bits(a if layout == "tf" else train_step.to_tf_layout(n, a))), key
    for n, _s in SMALL_STATS:
        assert np.array_equal(stored[n], S1[n].cpu().numpy())

    P2, S2 = _small_model(cuda, 59)                     # other values everywhere: restore must overwrite all of them
    t2 = ssd.TrainStep(P2, CFG, statistics=S2, layout=layout)
    assert t2.restore(str(tmp_path / "run")) == prefix and t2.global_step == 3
    for n, _s in SMALL_STATS:
        assert cuda.equal(S2[n], S1[n])
    _drive(cuda, t2, P2, grads[3:])
    assert t2.global_step == 5
    _assert_same_bits(_read(t2, P2), want, [n for n, _ in SMALL])


def test_thirty_steps_of_a_torch_head_then_the_checkpoint_feeds_the_library(ssd, cuda, tmp_path):
    """End to end on one fixed synthetic batch: the whole MobileNet variable set sits in TrainStep (torch layout); the two final head
    layers act as 1x1 heads -- the centre tap of their 3x3 kernels as a matmul over fixed random features, so nothing depends on a
    convolution library -- and are the only tensors with gradients.  differentiable_loss + step() for 30 steps lower the loss, and
    the saved checkpoint gives load_ckpt_weights(use_ema=True) exactly ema(name) in TF layout."""
    from ssd_amd import train_step
    torch = cuda
    W = ssd.synthetic_weights(MOBILENET, seed=60)
    names = train_step.trainable_names(MOBILENET)
    P = {n: torch.from_numpy(train_step.from_tf_layout(n, W[n])).cuda().requires_grad_(True) for n in names}
    S = {n: torch.from_numpy(W[n]).cuda() for n in W if n not in P}
    cfg = {"initial_learning_rate": 0.01, "num_steps": 1000, "weight_decay": 5e-5}
    ts = ssd.TrainStep(P, cfg, statistics=S, layout="torch", params=MOBILENET)
    g = ssd.AnchorGenerator()
    anchors = g(128, 256)
    N, C = len(anchors), 80
    assert N % 6 == 0
    rng = np.random.default_rng(61)
    B = 2
    feats = torch.from_numpy(rng.normal(0, 1.0 / 16.0, (B, N // 6, 256)).astype(np.float32)).cuda()
    counts = [6, 3]
    boxes = np.zeros((B, 6, 4), np.float32)
    for b, n in enumerate(counts):                                              # ground truth = anchors, shifted and resized a little
        k = anchors[rng.integers(0, N, n)].astype(np.float64)
        h, w = k[:, 2] - k[:, 0], k[:, 3] - k[:, 1]
        cy, cx = (k[:, 0] + k[:, 2]) / 2 + 0.08 * h, (k[:, 1] + k[:, 3]) / 2 - 0.05 * w
        h, w = h * 1.15, w * 0.9
        boxes[b, :n] = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
    gt = {"boxes": boxes, "labels": rng.integers(0, C, (B, 6)).astype(np.int32), "num_boxes": np.array(counts, np.int32)}
    a = torch.from_numpy(anchors).cuda()
    LP = {"gamma": 2.0, "alpha": 0.25}
    kc, bc = P["class_net/logits/kernel"], P["class_net/logits/bias"]             # [480, 256, 3, 3], [480]
    kb, bb = P["box_net/encoded_boxes/kernel"], P["box_net/encoded_boxes/bias"]   # [24, 256, 3, 3], [24]
    totals = []
    for _ in range(31):
        logits = (feats @ kc[:, :, 1, 1].t() + bc).reshape(B, N, C)
        codes = (feats @ kb[:, :, 1, 1].t() + bb).reshape(B, N, 4)
        out = ssd.differentiable_loss(logits, codes, a, gt, LP)
        total = out["localization_loss"] + 2.0 * out["classification_loss"]
        totals.append(float(total.item()))
        if len(totals) == 31:
            break
        for p in (kc, bc, kb, bb):
            p.grad = None
        total.backward()
        ts.step()
    print("total loss at steps 0, 10, 20, 30:", totals[0], totals[10], totals[20], totals[30])
    assert ts.global_step == 30
    assert np.isfinite(totals).all() and totals[30] < totals[0], totals
    untouched = "MobilenetV1/Conv2d_0/weights"                                    # no gradient: w kept, ema == w
    assert np.array_equal(P[untouched].detach().cpu().numpy(), train_step.from_tf_layout(untouched, W[untouched]))
    assert torch.equal(ts.ema(untouched), P[untouched].detach())
    assert not torch.equal(ts.ema("class_net/logits/kernel"), kc.detach()) and not torch.equal(kc.detach().cpu(), torch.from_numpy(
        train_step.from_tf_layout("class_net/logits/kernel", W["class_net/logits/kernel"])))
    model_dir = str(tmp_path / "run")
    ts.save(model_dir)
    ema = ssd.load_ckpt_weights(model_dir, MOBILENET, use_ema=True)
    raw = ssd.load_ckpt_weights(model_dir, MOBILENET, use_ema=False)
    assert list(ema) == list(W)
    for n in W:
        if n in P:
            assert ema[n].shape == W[n].shape
            assert np.array_equal(_bits(ema[n]), _bits(train_step.to_tf_layout(n, ts.ema(n).cpu().numpy()))), n
            assert np.array_equal(_bits(raw[n]), _bits(train_step.to_tf_layout(n, P[n].detach().cpu().numpy()))), n
        else:
            assert np.array_equal(ema[n], W[n]) and np.array_equal(raw[n], W[n]), n
