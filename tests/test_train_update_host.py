"""The TRAIN update without a GPU: the numpy restatement against torch.optim.Adam and its own float64 form, the host scalars,
the weight-decay selection, ssd_train_update's refusals, and the checkpoint writer through the package's reader."""
import ctypes
import math
import os

import numpy as np
import pytest

from helpers import train_update_ref as ref

CFG = {"initial_learning_rate": 1e-3, "num_steps": 1000, "weight_decay": 5e-5}
MOBILENET = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
SHUFFLENET = {"backbone": "shufflenet", "depth_multiplier": 1.0, "num_classes": 80}


def _state(rng, n, dtype):
    w = rng.uniform(-4, 4, n).astype(dtype)
    return [w, np.zeros(n, dtype), np.zeros(n, dtype), w.copy()]


def test_float64_restatement_equals_torch_adam_without_epsilon_and_differs_with_it():
    import torch
    rng = np.random.default_rng(0)
    w0 = rng.uniform(-4, 4, 1000)
    grads = [rng.normal(0, 1, 1000) for _ in range(5)]
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 10 ** 9, "weight_decay": 0.0}       # the cosine factor stays 1 to 1e-17

    def torch_adam(eps):
        p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([p], lr=float(np.float32(1e-3)), betas=(0.9, 0.999), eps=eps)
        for g in grads:
            p.grad = torch.tensor(g, dtype=torch.float64)
            opt.step()
        return p.detach().numpy()

    def ours(eps):
        s = [w0.copy(), np.zeros(1000), np.zeros(1000), w0.copy()]
        ref.run(cfg, [s], [[g] for g in grads], [False], epsilon=eps)
        return s[0]
    d0 = np.abs(ours(0.0) - torch_adam(0.0)).max()
    print("epsilon 0: max |ours - torch| = %.3g" % d0)
    assert d0 <= 1e-12
    d8 = np.abs(ours(1e-8) - torch_adam(1e-8)).max()
    print("epsilon 1e-8: max |ours - torch| = %.3g" % d8)
    assert d8 > 0.0            # "epsilon hat" (outside the bias correction) is not torch's epsilon


def test_float32_restatement_stays_within_S_ulps_of_the_float64_one():
    rng = np.random.default_rng(1)
    S, n = 5, 1000
    s32 = _state(rng, n, np.float32)
    s64 = [a.astype(np.float64) for a in s32]
    grads = [rng.normal(0, 1, n).astype(np.float32) for _ in range(S)]
    ref.run(CFG, [s32], [[g] for g in grads], [True])
    ref.run(CFG, [s64], [[g.astype(np.float64)] for g in grads], [True])
    bound = S * float(np.spacing(np.float32(np.abs(s64[0]).max())))
    err = np.abs(s32[0].astype(np.float64) - s64[0]).max()
    print("float32 vs float64 after %d steps: %.3g (bound %.3g)" % (S, err, bound))
    assert err <= bound


def test_learning_rate_and_ema_decay_known_answers(ssd):
    from ssd_amd import train_step
    cfg = {"initial_learning_rate": 1e-4, "num_steps": 350000, "weight_decay": 5e-5}
    for mod in (ref, train_step):
        assert mod.learning_rate(cfg, 0) == 1e-4
        assert abs(mod.learning_rate(cfg, 175000) - 0.5e-4) <= 1e-19
        assert abs(mod.learning_rate(cfg, 350000)) <= 1e-19
        assert mod.learning_rate(cfg, 350001) == mod.learning_rate(cfg, 350000) == mod.learning_rate(cfg, 10 ** 7)
        assert mod.ema_decay(1) == 2.0 / 11.0
        assert mod.ema_decay(1275) < 0.993 and mod.ema_decay(1276) == 0.993 == mod.ema_decay(10 ** 6)
        assert [t for t in range(1, 2000) if (1.0 + t) / (10.0 + t) >= 0.993][0] == 1276
    # the package's scalars are the helper's, bit for bit
    for t in (1, 2, 10, 1276, 350000, 400000):
        s = train_step.step_scalars(cfg, t)
        got = np.array([s.alpha, s.one_minus_beta1, s.one_minus_beta2, s.epsilon, s.weight_decay, s.one_minus_decay], np.float32)
        assert np.array_equal(got.view(np.uint32), np.array(ref.scalars(cfg, t), np.float32).view(np.uint32)), t
    assert ssd.load_optimizer_config(dict(cfg, backbone="mobilenet")) == cfg and ssd.OPTIMIZER_KEYS == tuple(cfg)
    with pytest.raises(KeyError):
        ssd.load_optimizer_config({"num_steps": 3, "weight_decay": 0.0})


def test_ema_closed_form_for_a_constant_variable():
    # w constant (NULL gradient): ema_t - w = (ema_0 - w) * prod(d_k), d_k = min(0.993, (1 + k) / (10 + k))
    w = np.full(4, 2.0)
    s = [w.copy(), np.zeros(4), np.zeros(4), np.full(4, 5.0)]
    ref.run(CFG, [s], [[None]] * 40, [False])
    prod = math.prod(ref.ema_decay(k) for k in range(1, 41))
    assert np.abs(s[3] - (2.0 + 3.0 * prod)).max() <= 1e-14
    assert np.array_equal(s[0], w)


def test_null_gradient_keeps_w_m_v_and_moves_ema():
    rng = np.random.default_rng(2)
    s = _state(rng, 64, np.float32)
    s[1][:] = 0.25
    s[2][:] = 0.5
    s[3] += np.float32(1.0)
    before = [a.copy() for a in s]
    ref.run(CFG, [s], [[None]], [True])
    assert all(np.array_equal(a, b) for a, b in zip(s[:3], before[:3]))
    assert not np.array_equal(s[3], before[3])
    assert np.array_equal(s[3], before[3] - (before[3] - s[0]) * np.float32(1.0 - 2.0 / 11.0))


@pytest.mark.parametrize("params,selected,total", [(MOBILENET, 32, 191), (SHUFFLENET, 55, 278)])
def test_weight_decay_selection_counts(ssd, params, selected, total):
    from ssd_amd import train_step
    names = train_step.trainable_names(params)
    assert len(names) == total
    assert sum(train_step.decays(n) for n in names) == selected == sum(ref.decays(n) for n in names)
    shapes = ssd.variable_shapes(params)
    assert sum(int(np.prod(shapes[n])) for n in names) == {191: 14287672, 278: 12223550}[total]


def test_ssd_train_update_refuses_bad_arguments_without_a_gpu(ssd):
    from ssd_amd import train_step, _lib
    L = ssd.lib()
    rows = np.zeros(3, train_step.TENSOR_DTYPE)
    for c in ("w", "grad", "m", "v", "ema"):
        rows[c] = 0x10000                       # never dereferenced: every refusal comes before any HIP call
    rows["count"] = (5000, 10, 4096)
    rows["decay"] = (1, 0, 0)
    rows["first_block"] = (0, 2, 3)
    good = (0.1, 0.1, 0.001, 1e-8, 5e-5, 0.5)
    fake = ctypes.c_void_p(0x20000)

    def call(r=rows, dev=fake, T=3, sc=good):
        s = _lib.SsdUpdateScalars(*sc) if sc is not None else None
        return L.ssd_train_update(r.ctypes.data_as(ctypes.c_void_p) if r is not None else None, dev, T,
                                  ctypes.byref(s) if s is not None else None, None)
    for kw in ({"r": None}, {"dev": None}, {"sc": None}, {"T": 0}, {"T": -1}, {"dev": ctypes.c_void_p(0x20004)},
               {"sc": (float("nan"),) + good[1:]}, {"sc": good[:5] + (float("inf"),)}, {"sc": good[:3] + (float("-inf"),) + good[4:]}):
        assert call(**kw) == -1, kw
        assert L.ssd_last_error().decode().startswith("ssd_train_update"), kw
    for field, value, word in (("count", -1, "count"), ("w", 0, "NULL"), ("m", 0, "NULL"), ("v", 0, "NULL"), ("ema", 0, "NULL"),
                               ("w", 0x10002, "aligned"), ("m", 0x10001, "aligned"), ("v", 0x10003, "aligned"),
                               ("ema", 0x10002, "aligned"), ("grad", 0x10002, "aligned"), ("decay", 2, "decay"),
                               ("first_block", 1, "first_block")):
        q = rows.copy()
        q[1][field] = value
        assert call(r=q) == -1, field
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_train_update") and "tensor 1" in msg and word in msg, (field, msg)
    # a w that starts inside a 16-byte group counts its blocks from the group's start: 2 + 4094 elements are ONE block, 2 + 4095 two
    q = rows.copy()
    q[0]["w"], q[0]["count"] = 0x10008, 4094
    assert call(r=q) == -1 and "tensor 1: first_block must be 1" in L.ssd_last_error().decode()
    q[0]["count"] = 4095
    assert train_step.block_starts(q["w"], q["count"])[0].tolist() == [0, 2, 3]


def test_the_five_table_entry_points_refuse_alike_and_in_one_order(ssd):
    """ssd_train_update, ssd_train_norms, ssd_train_histograms and the two planners check one table: the same text behind the
    function's name for a spoilt row, ssd_train_update's order where two faults meet, and no refusal of a table of empty rows."""
    from ssd_amd import train_step, _lib
    L = ssd.lib()
    rows = np.zeros(3, train_step.TENSOR_DTYPE)
    for c in ("w", "grad", "m", "v", "ema"):
        rows[c] = 0x10000                       # never dereferenced: every refusal comes before any HIP call
    rows["count"] = (5000, 10, 4096)
    rows["decay"] = (1, 0, 0)
    rows["first_block"] = (0, 2, 3)
    good = (0.1, 0.1, 0.001, 1e-8, 5e-5, 0.5)
    fake, out = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)

    def p(r):
        return r.ctypes.data_as(ctypes.c_void_p) if r is not None else None

    def update(r, T=3, sc=good, dev=fake):
        s = _lib.SsdUpdateScalars(*sc) if sc is not None else None
        return L.ssd_train_update(p(r), dev, T, ctypes.byref(s) if s is not None else None, None)
    entry = {"ssd_train_update": update,
             "ssd_train_norms": lambda r, T=3: L.ssd_train_norms(p(r), fake, T, out, out, fake, 1 << 20, None),
             "ssd_train_norms_workspace_bytes": lambda r, T=3: -1 if L.ssd_train_norms_workspace_bytes(p(r), T) == 0 else 0,
             "ssd_train_histograms": lambda r, T=3: L.ssd_train_histograms(p(r), fake, T, 1e-4, out, out, out, fake, 1 << 20, None),
             "ssd_train_histograms_workspace_bytes": lambda r, T=3: -1 if L.ssd_train_histograms_workspace_bytes(p(r), T) == 0 else 0}
    # one bad row at a time through all five: the text behind the function's name is one
    for t in range(3):
        for field, value, text in (("count", -1, "bad count"), ("m", 0, "NULL w, m, v or ema"),
                                   ("w", 0x10002, "w, m, v, ema and grad must be 4-byte aligned"), ("decay", 2, "decay must be 0 or 1"),
                                   ("first_block", 7, "first_block must be %d" % rows["first_block"][t])):
            q = rows.copy()
            q[t][field] = value
            for name, fn in entry.items():
                assert fn(q) == -1, (name, t, field)
                head, _, tail = L.ssd_last_error().decode().partition(": ")
                assert head == name and tail == "tensor %d: %s" % (t, text), (name, t, field, head, tail)
    # two faults at once in ssd_train_update: which one wins
    nan = (float("nan"),) + good[1:]
    bad = rows.copy()
    bad[0]["count"] = -1
    assert update(bad, sc=nan) == -1 and L.ssd_last_error().decode() == "ssd_train_update: non-finite scalar"
    assert update(rows, T=0, sc=nan) == -1 and L.ssd_last_error().decode() == "ssd_train_update: T must be in [1, 65536]"
    for kw in ({"r": bad}, {"r": rows, "T": 0}, {"r": rows, "dev": ctypes.c_void_p(0x20004)}, {"r": None}, {"r": rows, "dev": None}):
        assert update(sc=None, **kw) == -1 and L.ssd_last_error().decode() == "ssd_train_update: bad arguments", kw
    assert update(rows, dev=ctypes.c_void_p(0x20004), sc=nan) == -1
    assert L.ssd_last_error().decode() == "ssd_train_update: tensors_dev must be 8-byte aligned"
    # a table of empty rows only: nothing to refuse, no block, no workspace byte
    empty = rows.copy()
    empty["count"], empty["first_block"] = 0, 0
    assert update(empty) == 0
    assert L.ssd_train_norms_workspace_bytes(p(empty), 3) == 0 == L.ssd_train_histograms_workspace_bytes(p(empty), 3)
    # norms and histograms still launch their stage 2 for such a table (it writes the outputs: zeros).  Where there is a GPU they
    # get real memory and return SSD_OK; where there is none, the launch's error -- not a refusal -- shows that every check passed
    import torch
    if not torch.cuda.is_available():
        for name in ("ssd_train_norms", "ssd_train_histograms"):
            assert entry[name](empty) == -2 and L.ssd_last_error().decode().startswith("hipGetLastError()"), name
        return
    from ssd_amd import train_calls
    host = torch.from_numpy(empty.view(np.uint8).copy())
    dev = host.cuda()
    sums = torch.full((3, 2), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.full((3, 2), -1, dtype=torch.int64, device="cuda")
    train_calls.train_norms(host, dev, sums, bad)                     # raises on any code but SSD_OK
    assert not sums.cpu().numpy().view(np.int64).any() and not bad.cpu().numpy().any()
    limits = train_calls.histogram_limits()
    counts = torch.full((3, 2, len(limits)), -1, dtype=torch.int64, device="cuda")
    stats = torch.full((3, 2, train_calls.STATS_BYTES), 255, dtype=torch.uint8, device="cuda")
    train_calls.train_histograms(host, dev, 1e-4, torch.from_numpy(limits.copy()).cuda(), counts, stats)
    got = stats.cpu().numpy().view(train_calls.STATS_DTYPE)
    assert not counts.cpu().numpy().any() and not got["num"].any() and not got["bad"].any() and not got["sum"].any()


def _weights(ssd, params):
    W = ssd.synthetic_weights(params, seed=3)
    rng = np.random.default_rng(4)
    out = dict(W)
    from ssd_amd import train_step
    for n in train_step.trainable_names(params):
        out[n + "/ExponentialMovingAverage"] = (W[n] + rng.normal(0, 0.01, W[n].shape)).astype(np.float32)
    out["global_step"] = np.int64(1234)
    return W, out


def test_ckpt_export_round_trip_dtypes_scalars_and_many_blocks(ssd, tmp_path):
    from ssd_amd import ckpt_export, ckpt_import
    rng = np.random.default_rng(5)
    T = {"a/float": rng.normal(0, 1, (3, 4, 5)).astype(np.float32), "global_step": np.int64(77), "scalar32": np.float32(2.5),
         "ints": np.arange(-3, 9, dtype=np.int64).reshape(3, 4), "empty_dim": np.zeros((0, 3), np.float32)}
    for i in range(400):
        T["layer_%03d/BatchNorm/gamma" % i] = rng.normal(0, 1, i % 7 + 1).astype(np.float32)
    prefix = ckpt_export.write_checkpoint(str(tmp_path / "model.ckpt-77"), T, block_bytes=2048)
    raw = open(prefix + ".index", "rb").read()
    table = ckpt_import.read_table(prefix + ".index", verify=True)
    assert len(table) == len(T) + 1 and list(table) == sorted(table)
    assert len(raw) > 6 * 2048                  # several data blocks of ~50 entries: the index block and the restart points are in use
    got = ckpt_import.read_checkpoint(prefix, verify=True)
    assert set(got) == set(T)
    for k, v in T.items():
        v = np.asarray(v)
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), k
    # one block (the default block size) reads the same
    p1 = ckpt_export.write_checkpoint(str(tmp_path / "one.ckpt-1"), T)
    g1 = ckpt_import.read_checkpoint(p1, verify=True)
    assert all(np.array_equal(g1[k], got[k]) for k in T)
    with pytest.raises(ValueError):
        ckpt_export.write_checkpoint(str(tmp_path / "bad"), {"x": np.zeros(3, np.complex64)})


@pytest.mark.parametrize("params", [MOBILENET, SHUFFLENET], ids=["mobilenet", "shufflenet"])
def test_ckpt_export_feeds_load_ckpt_weights_raw_and_ema(ssd, tmp_path, params):
    from ssd_amd import ckpt_export
    W, out = _weights(ssd, params)
    model_dir = str(tmp_path / "run")
    os.makedirs(model_dir)
    ckpt_export.write_checkpoint(os.path.join(model_dir, "model.ckpt-1234"), out)
    ckpt_export.write_checkpoint_state(model_dir, "model.ckpt-1234")
    assert ssd.resolve_checkpoint(model_dir) == os.path.join(model_dir, "model.ckpt-1234")
    raw = ssd.load_ckpt_weights(model_dir, params, use_ema=False)
    ema = ssd.load_ckpt_weights(model_dir, params, use_ema=True)
    assert list(raw) == list(W) == list(ema)
    n_ema = 0
    for n in W:
        assert np.array_equal(raw[n], W[n]), n
        src = out.get(n + "/ExponentialMovingAverage")
        n_ema += src is not None
        assert np.array_equal(ema[n], W[n] if src is None else src), n
    assert n_ema == (191 if params is MOBILENET else 278)


def test_ckpt_export_flipped_data_byte_is_caught(ssd, tmp_path):
    from ssd_amd import ckpt_export, ckpt_import
    T = {"a": np.arange(100, dtype=np.float32), "b": np.arange(50, dtype=np.float32)}
    prefix = ckpt_export.write_checkpoint(str(tmp_path / "m.ckpt-0"), T)
    path = prefix + ".data-00000-of-00001"
    raw = bytearray(open(path, "rb").read())
    raw[417] ^= 0x10                            # inside "b"
    open(path, "wb").write(raw)
    assert np.array_equal(ckpt_import.read_checkpoint(prefix, ["a"], verify=True)["a"], T["a"])
    with pytest.raises(ValueError, match="checksum"):
        ckpt_import.read_checkpoint(prefix, ["b"], verify=True)
    # ... and a flipped byte of the index by the block checksum
    ix = bytearray(open(prefix + ".index", "rb").read())
    ix[5] ^= 0x01
    open(prefix + ".index", "wb").write(ix)
    with pytest.raises(ValueError, match="checksum"):
        ckpt_import.read_checkpoint(prefix, verify=True)


def test_layout_transposes_are_inverse_and_match_tf_shapes(ssd):
    from ssd_amd import train_step
    rng = np.random.default_rng(6)
    k = rng.normal(0, 1, (8, 5, 3, 3)).astype(np.float32)                    # OIHW
    hwio = train_step.to_tf_layout("fpn/p3/kernel", k)
    assert hwio.shape == (3, 3, 5, 8) and hwio[1, 2, 4, 7] == k[7, 4, 1, 2]
    assert np.array_equal(train_step.from_tf_layout("fpn/p3/kernel", hwio), k)
    d = rng.normal(0, 1, (6, 1, 3, 3)).astype(np.float32)                    # depthwise [C,1,k,k]
    tf = train_step.to_tf_layout("x/depthwise_weights", d)
    assert tf.shape == (3, 3, 6, 1) and tf[2, 0, 5, 0] == d[5, 0, 2, 0]
    assert np.array_equal(train_step.from_tf_layout("x/depthwise_weights", tf), d)
    b = rng.normal(0, 1, 7).astype(np.float32)
    assert train_step.to_tf_layout("box_net/logits/bias", b) is b
