"""ssd_loss_top_means on the GPU against helpers/loss_top_ref.py, bit for bit (include/ssd_hip.h, "the per-level top
losses"), on the smallest shapes at which the kernels can go wrong: ties across rank k, the tail of zeros of a localisation plane,
-0.0 below +0.0, k = 1, one level past a power of two and one of the training shape's largest, non-finite values and denormals at segment
ends and at rank k, rows and levels at 4-byte-only addresses, B = 1, more segments than one grid pass; every tensor of the call in
one guarded arena; a second launch and a side stream; and the Trainer's ten histograms end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import example_protos, guarded
from helpers import histogram_ref as hist_ref
from helpers import loss_top_ref as ref
from helpers.head_train_gpu import same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
SMALL = (150, 37, 5, 1, 1)


# ----------------------------------------------------------------------------- the cases: name -> (levels, planes [2, B, N])
def _ties(levels, B, seed):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.standard_normal(38).astype(f32), f32([0.0, -0.0])])       # 40 distinct numbers: ties everywhere
    return pool[rng.integers(0, 40, (2, B, sum(levels)))]


def _loc_like(shape, seed):
    """97 % exact +0.0, a few -0.0, the rest positive: fewer non-zeros than k = n / 5."""
    rng = np.random.default_rng(seed)
    x = np.zeros(shape, f32)
    u = rng.random(shape)
    x[u < 0.02] = rng.random(int((u < 0.02).sum())).astype(f32) * f32(3)
    x[u > 0.99] = f32(-0.0)
    return x


def _case_zeros():
    levels = (1000, 150, 37)
    planes = _loc_like((2, 2, sum(levels)), 3)
    # level 2 of image 0, plane 1 (n = 37, k = 8): three positives, two +0.0, the rest -0.0 -- the top ends in three -0.0
    seg = np.full(37, -0.0, f32)
    seg[[0, 17, 36]] = f32([0.5, 2.0, 0.25])
    seg[[5, 30]] = f32(0.0)
    planes[1, 0, 1150:] = seg
    return levels, planes


def _case_equal():
    return (300, 7), np.full((2, 2, 307), 0.25, f32)


def _case_k1():
    rng = np.random.default_rng(5)
    return (1, 2, 3, 4, 5), rng.standard_normal((2, 2, 15)).astype(f32)


def _case_large():
    levels = (38400, 40961)                                # k = 7680: pad 8192, 38 strides of the block | k = 8193: the first past 8192
    rng = np.random.default_rng(6)
    planes = np.stack([rng.standard_normal((2, sum(levels))).astype(f32), _loc_like((2, sum(levels)), 7)])
    planes[0, 1, :38400] = np.round(planes[0, 1, :38400] * f32(8)) / f32(8)      # ... and one dense segment of heavy ties
    return levels, planes


def _case_specials():
    """Bit patterns, so that no conversion touches a signalling NaN.  Everything not set below is a negative normal number."""
    levels = (41, 10, 64)                                  # k = 9, 2, 13; offsets 0, 41, 51
    rng = np.random.default_rng(8)
    planes = -np.abs(rng.standard_normal((2, 2, sum(levels)))).astype(f32) - f32(0.5)
    bits = planes.view(u32)
    a = bits[0, 0]
    a[0], a[40] = 0xFFC00000, 0xFF800000                   # level 0: -NaN first, -inf last
    for i, v in ((3, 0x7F800001), (7, 0x7F800000), (11, 0x7F7FFFFF), (13, 0x7FC00000), (23, 0x3F800000), (29, 0x40000000),
                 (17, 0x007FFFFF), (19, 0x007FFFFF), (31, 0x007FFFFF), (37, 0x007FFFFF), (33, 0x00000000), (35, 0x80000000)):
        a[i] = v                                           # six keys above the largest denormal; ranks 7 .. 10 are four equal denormals:
    a[41], a[50] = 0x7FC00000, 0x7F800000                  # rank 9 cuts the tie.  Level 1: +NaN first, +inf last = rank k
    a[51], a[114] = 0xFF7FFFFF, 0xFFFFFFFF                 # level 2: -FLT_MAX first, the lowest key of all last
    b = bits[1, 1]
    b[:41] = 0xFF7FFFFF                                    # level 0: rank k inside a run of -FLT_MAX
    b[0], b[40], b[5], b[6] = 0xFF800000, 0xFFC00000, 0x00000001, 0x80000001
    b[41:49], b[49], b[50] = 0xFF800000, 0xFFC00000, 0xFFFFFFFF      # level 1: -inf eight times above both -NaN
    b[51:] = 0x7F800000                                    # level 2: +inf everywhere, a +NaN on either end
    b[51], b[114] = 0x7FC00000, 0x7F800001
    c = bits[0, 1]                                         # image 1 of plane 0: a finite value meets the NaN slots, FLT_MAX the +inf slot
    c[0], c[40], c[45] = 0x00000001, 0x7F7FFFFF, 0x7F7FFFFF
    return levels, planes


CASES = {
    "ties": lambda: (SMALL, _ties(SMALL, 3, 1)),
    "zeros": _case_zeros,
    "equal": _case_equal,
    "k1": _case_k1,
    "large": _case_large,
    "specials": _case_specials,
    "specials_b1": lambda: (_case_specials()[0], _case_specials()[1][:, :1]),           # B = 1: a denormal's mean is the denormal
    "odd": lambda: ((151, 37, 5, 3, 1), _ties((151, 37, 5, 3, 1), 3, 2)),          # N = 197: every row but the first at 4 (mod 16)
    "batch1": lambda: (SMALL, _ties(SMALL, 1, 9)),
    "many": lambda: ((7, 6, 5, 4, 3, 2, 1, 9), _ties((7, 6, 5, 4, 3, 2, 1, 9), 150, 4)),     # 2400 segments: more than one grid pass
}
_made = {}


def _case(name):
    """(levels, planes, V, M) of a case: made once, shared, never written."""
    if name not in _made:
        levels, planes = CASES[name]()
        planes = np.ascontiguousarray(planes, f32)
        out = (levels, planes, ref.selected(planes, levels), ref.means(planes, levels))
        for a in out[1:]:
            a.setflags(write=False)
        _made[name] = out
    return _made[name]


def _launch(ssd, torch, levels, planes, contract=16, stream=None, layout="skewed", twice=False):
    """One call inside a guarded arena -> (means [2,K], V [2,B,K]) as read back, after the guards were checked."""
    L = ssd.lib()
    _, B, N = planes.shape
    K = sum(ref.counts(levels))
    arena = guarded.Arena(torch, torch.device("cuda", 0), layout)
    arena.add("cls", planes[0].copy(), f32, contract, "input")
    arena.add("loc", planes[1].copy(), f32, contract, "input")
    arena.add("means", (2, K), f32, contract, "output")
    arena.add("workspace", (2 * B * K * 4,), np.uint8, 16, "workspace")
    lv = (ctypes.c_int64 * len(levels))(*levels)
    need = L.ssd_loss_top_workspace_bytes(B, lv, len(levels))
    assert need == 2 * B * K * 4
    if layout == "skewed":
        assert arena.ptr("workspace") % 32 == 16 and (contract != 16 or arena.ptr("cls") % 32 == 16 == arena.ptr("means") % 32)
    s = torch.cuda.current_stream() if stream is None else stream
    for _ in range(2 if twice else 1):
        ssd._lib.check(L.ssd_loss_top_means(arena.ptr("cls"), arena.ptr("loc"), B, N, lv, len(levels), arena.ptr("means"),
                                            arena.ptr("workspace"), need, ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    arena.check()
    return arena.read("means"), arena.read("workspace").view(f32).reshape(2, B, K)


def _assert_case(name, means, V):
    levels, planes, want_V, want_M = _case(name)
    assert np.array_equal(V.view(u32), want_V.view(u32)), name                  # every workspace element written, every bit
    if name.startswith("specials"):                                              # which quiet NaN a sum over a NaN gives is not pinned
        assert ref.same_bits(means, want_M) and np.isnan(want_M).any(), name
    else:
        assert not np.isnan(want_M).any() and np.array_equal(means.view(u32), want_M.view(u32)), name


@pytest.mark.parametrize("contract", [16, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_restatement_bit_for_bit(ssd, cuda, name, contract):
    levels, planes, _V, _M = _case(name)
    means, V = _launch(ssd, cuda, levels, planes, contract)
    _assert_case(name, means, V)


def test_the_tail_of_zeros_and_the_order_of_minus_zero(ssd, cuda):
    levels, planes, _V, _M = _case("zeros")
    _means, V = _launch(ssd, cuda, levels, planes)
    ks = ref.counts(levels)
    tail = V[1, 0, ks[0] + ks[1]:]                                               # the crafted segment: 2.0, 0.5, 0.25, +0.0 x2, -0.0 x3
    assert np.array_equal(tail.view(u32), f32([2.0, 0.5, 0.25, 0.0, 0.0, -0.0, -0.0, -0.0]).view(u32))
    for p, b in ((1, 0), (1, 1), (0, 1)):
        seg, top = planes[p, b, :1000], V[p, b, :ks[0]]
        g = int((seg > 0).sum())
        assert 0 < g < ks[0] and np.all(top[:g] > 0) and np.all(np.diff(top[:g]) <= 0)
        assert np.array_equal(top[g:].view(u32), np.zeros(ks[0] - g, u32))       # the rest of the k slots: exact +0.0, no -0.0
    levels, planes, _V, _M = _case("specials_b1")
    means, V = _launch(ssd, cuda, levels, planes)
    top9 = np.array([0x7FC00000, 0x7F800001, 0x7F800000, 0x7F7FFFFF, 0x40000000, 0x3F800000, 0x007FFFFF, 0x007FFFFF, 0x007FFFFF], u32)
    assert np.array_equal(V[0, 0, :9].view(u32), top9)                           # both NaNs keep their bits in V
    assert np.array_equal(V[0, 0, 9:11].view(u32), np.array([0x7FC00000, 0x7F800000], u32))
    assert np.isnan(means[0, :2]).all() and np.array_equal(means[0, 2:9].view(u32), top9[2:])     # x / 1: the denormals keep every bit
    levels, planes, _V, _M = _case("specials")
    _means, V = _launch(ssd, cuda, levels, planes)
    assert np.array_equal(V[1, 1, :11].view(u32), np.array([0x00000001, 0x80000001] + [0xFF7FFFFF] * 7 + [0xFF800000] * 2, u32))
    assert np.array_equal(V[1, 1, 11:13].view(u32), np.array([0x7FC00000, 0x7F800001], u32))


def test_a_second_launch_and_a_side_stream_give_the_same_bytes(ssd, cuda):
    for name in ("ties", "large"):
        levels, planes, _V, _M = _case(name)
        once = _launch(ssd, cuda, levels, planes)
        again = _launch(ssd, cuda, levels, planes, twice=True)
        side = cuda.cuda.Stream()
        cuda.cuda.synchronize()
        with cuda.cuda.stream(side):
            other = _launch(ssd, cuda, levels, planes, stream=side, layout="aligned")
        for got in (once, again, other):
            _assert_case(name, *got)
            assert got[0].tobytes() == once[0].tobytes() and got[1].tobytes() == once[1].tobytes()


def test_the_public_call_and_the_call_layer(ssd, cuda):
    from ssd_amd import train_calls
    levels, planes, _V, want = _case("odd")
    dev = cuda.device("cuda", 0)
    cls, loc = cuda.from_numpy(planes[0].copy()).to(dev), cuda.from_numpy(planes[1].copy()).to(dev)
    means, counts = ssd.level_top_means(cls, loc, levels)
    assert counts == tuple(ref.counts(levels)) and tuple(means.shape) == (2, sum(counts))
    assert np.array_equal(means.cpu().numpy().view(u32), want.view(u32))
    ws = cuda.empty(train_calls.loss_top_workspace_bytes(3, levels), dtype=cuda.uint8, device=dev)
    out = cuda.full((2, sum(counts)), float("nan"), device=dev)
    train_calls.loss_top_means(cls, loc, levels, out, workspace=ws)
    assert np.array_equal(out.cpu().numpy().view(u32), want.view(u32))
    with pytest.raises(ssd.SsdError, match="workspace too small"):
        train_calls.loss_top_means(cls, loc, levels, out, workspace=ws[:-16])
    with pytest.raises(ssd.SsdError, match="sum to 196 anchors, N is 197"):
        train_calls.loss_top_means(cls, loc, (150, 37, 5, 3, 1), cuda.empty((2, 41), device=dev))


# ----------------------------------------------------------------------------- the Trainer, end to end
SEED = 40                               # test_gpu_trainer.py's: every image of the first batches keeps a box
BASE = dict(TINY_PARAMS, batch_size=2, image_height=128, image_width=128, initial_learning_rate=1e-3, num_steps=100, weight_decay=1e-4,
            gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0)
OLD_TAGS = {"loss", "regularization_loss", "localization_loss", "classification_loss", "learning_rate/learning_rate"} | \
           {"losses/loss_summaries/mean_matches_per_image_on_level_%d" % l for l in range(3, 8)} | \
           {"losses/loss_summaries/total_mean_matches_per_image"}
NEW_TAGS = ["losses/loss_summaries/%s_losses_on_level_%d" % (kind, l) for kind in ("classification", "localization") for l in range(3, 8)]


def _write_shard(directory, name, n, seed):
    from ssd_amd import tfrecords
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        H, W = int(rng.integers(90, 260)), int(rng.integers(90, 260))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        m = int(rng.integers(1, 4))
        c = rng.uniform(0.1, 0.6, (m, 2))
        boxes = np.concatenate([c, c + rng.uniform(0.15, 0.35, (m, 2))], 1).clip(0, 1)
        recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, m)))
    os.makedirs(directory)
    tfrecords.write_records(os.path.join(directory, name), recs)
    return directory


@pytest.fixture(scope="module")
def data(ssd, tmp_path_factory):
    from ssd_amd import ckpt_export
    root = tmp_path_factory.mktemp("trainer_loss_top")
    out = {"train_dataset": _write_shard(str(root / "train"), "train-00.tfrecords", 24, 0),
           "val_dataset": _write_shard(str(root / "val"), "val-00.tfrecords", 4, 1)}
    W = ssd.synthetic_weights(TINY_PARAMS, seed=301, logits_bias=-4.0)
    out["mobilenet"] = ckpt_export.write_checkpoint(str(root / "mobilenet_pretrained.ckpt"),
                                                    {k: v for k, v in W.items() if k.startswith("MobilenetV1/")})
    return out


def _state(ts):
    out = {"statistic " + n: s.detach().cpu().numpy() for n, s in ts.statistics.items()}
    for n in ts.names:
        m, v = ts.slots(n)
        out.update({"variable " + n: ts.parameters[n].detach().cpu().numpy(), "average " + n: ts.ema(n).cpu().numpy(),
                    "m " + n: m.cpu().numpy(), "v " + n: v.cpu().numpy()})
    return out


def _events(ssd, directory):
    files = ssd.summaries.event_files(str(directory))
    return [e for f in files for e in ssd.summaries.read_events(f)], files


def test_the_trainer_writes_the_ten_histograms_and_changes_no_bit(ssd, cuda, data, tmp_path, monkeypatch):
    import ssd_amd.ssd as ssd_module

    def config(model_dir):
        return dict(BASE, backbone="mobilenet", model_dir=str(model_dir), train_dataset=data["train_dataset"],
                    val_dataset=data["val_dataset"], pretrained_checkpoint=data["mobilenet"])
    on = ssd.Trainer(config(tmp_path / "on"), seed=SEED, read_workers=2)
    off = ssd.Trainer(config(tmp_path / "off"), seed=SEED, read_workers=2)
    seen = []                                                                    # every loss call's per-anchor planes, as the step made them
    inner = ssd_module.differentiable_loss

    def spy(*args, **kwargs):
        out = inner(*args, **kwargs)
        seen.append(None if "cls_losses" not in out else np.stack([out["cls_losses"].cpu().numpy(), out["loc_losses"].cpu().numpy()]))
        return out
    monkeypatch.setattr(ssd_module, "differentiable_loss", spy)
    assert on.train(max_steps=2, log_every=1, save_summary_steps=1, loss_histograms=True) == 2
    assert len(seen) == 2 and all(s is not None for s in seen)
    assert off.train(max_steps=2, log_every=1, save_summary_steps=1) == 2
    assert seen[2:] == [None, None] and off._loss_top is None                    # off: nothing asked for, nothing allocated
    got, want = _state(on.train_step), _state(off.train_step)
    differ = [k for k in want if not same_bits(got[k], want[k])]
    assert set(got) == set(want) and not differ, differ[:5]

    events_on, _files = _events(ssd, tmp_path / "on")
    events_off, _files = _events(ssd, tmp_path / "off")
    assert [step for _w, step, _v in events_on] == [1, 2] == [step for _w, step, _v in events_off]
    levels = on.anchors_per_level
    ks = ref.counts(levels)
    K, L = sum(ks), len(levels)
    assert L == 5 and sum(levels) == seen[0].shape[2]
    base = on._loss_top["means"].data_ptr()
    for (_w, step, with_flag), (_w2, _s2, without), planes in zip(events_on, events_off, seen):
        plain = {t for t in without if not t.endswith("_hist")} - {"global_step/sec"}
        assert plain == OLD_TAGS
        assert {t for t in with_flag if not t.endswith("_hist")} - {"global_step/sec"} == OLD_TAGS | set(NEW_TAGS)
        assert {t for t in with_flag if t.endswith("_hist")} == {t for t in without if t.endswith("_hist")}
        M = ref.means(planes, levels)
        for p in range(2):
            koff = 0
            for l, k in enumerate(ks):
                h = with_flag[NEW_TAGS[p * L + l]]
                counts, st = hist_ref.plane(M[p, koff:koff + k], ((base + 4 * (p * K + koff)) // 4) % 4)
                lim, bkt = hist_ref.compressed(counts)
                assert h["num"] == float(st["num"]) == k, (step, p, l)
                assert h["min"] == float(st["min"]) and h["max"] == float(st["max"]), (step, p, l)
                assert h["sum"] == float(st["sum"]) and h["sum_squares"] == float(st["sum_squares"]), (step, p, l)
                assert h["bucket_limit"] == lim and h["bucket"] == bkt, (step, p, l)
                koff += k
        # the classification losses are positive everywhere; a level's localisation histogram is mostly the zero bucket
        assert all(with_flag[t]["min"] > 0 for t in NEW_TAGS[:5]) and all(with_flag[t]["min"] >= 0 for t in NEW_TAGS[5:])
    log = [json.loads(line) for line in open(tmp_path / "on" / "train_log.jsonl")]
    assert [r["step"] for r in log] == [1, 2]
