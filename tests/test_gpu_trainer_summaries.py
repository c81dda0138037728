"""ssd_amd.Trainer's TensorBoard summaries on the GPU: a run with summaries is bit for bit the run without them, the
event file holds one event per due step with the scalars of that step's log record and a histogram of every variable and gradient
that decodes to the numpy restatement (helpers/histogram_ref.py) of the variable, the schedule is SummarySaverHook's, the final
evaluation lands in model_dir/eval/, and a step that stops the run writes no event.  test_gpu_trainer.py's tiny configuration,
restated: TINY_PARAMS at 128 x 128, batch 2, on a 24-record shard and a 4-image validation shard."""
import json
import os

import numpy as np
import pytest

from helpers import example_protos
from helpers import histogram_ref as ref
from helpers.head_train_gpu import same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 40                               # test_gpu_trainer.py's: every image of the first batches keeps a box (asserted in _premises)
BASE = dict(TINY_PARAMS, batch_size=2, image_height=128, image_width=128, initial_learning_rate=1e-3, num_steps=100, weight_decay=1e-4,
            gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0)
SCALAR_TAGS = {"loss": "loss", "regularization_loss": "regularization_loss", "localization_loss": "localization_loss",
               "classification_loss": "classification_loss", "learning_rate/learning_rate": "learning_rate"}
MATCH_TAGS = ["losses/loss_summaries/mean_matches_per_image_on_level_%d" % l for l in range(3, 8)] + \
             ["losses/loss_summaries/total_mean_matches_per_image"]


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
    root = tmp_path_factory.mktemp("trainer_summaries")
    out = {"train_dataset": _write_shard(str(root / "train"), "train-00.tfrecords", 24, 0),
           "val_dataset": _write_shard(str(root / "val"), "val-00.tfrecords", 4, 1)}
    W = ssd.synthetic_weights(TINY_PARAMS, seed=301, logits_bias=-4.0)
    ckpt = {k: v for k, v in W.items() if k.startswith("MobilenetV1/")}
    out["mobilenet"] = ckpt_export.write_checkpoint(str(root / "mobilenet_pretrained.ckpt"), ckpt)
    return out


def _config(data, model_dir):
    return dict(BASE, backbone="mobilenet", model_dir=str(model_dir), train_dataset=data["train_dataset"], val_dataset=data["val_dataset"],
                pretrained_checkpoint=data["mobilenet"])


def _premises(ssd, data):
    from ssd_amd.trainer import pipeline_seed
    host = ssd.TrainPipeline(data["train_dataset"], BASE, seed=pipeline_seed(SEED, 0), read_workers=2).host_batches()
    for _ in range(5):
        kept = [len(labels) for _frame, _row, _boxes, labels in next(host)]
        assert len(kept) == 2 and min(kept) >= 1, kept
    host.close()


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


def test_summaries_change_no_bit_and_decode_to_the_restatement(ssd, cuda, data, tmp_path):
    _premises(ssd, data)
    on = ssd.Trainer(_config(data, tmp_path / "on"), seed=SEED, read_workers=2)
    off = ssd.Trainer(_config(data, tmp_path / "off"), seed=SEED, read_workers=2)
    initial = {n: p.detach().cpu().numpy().copy() for n, p in off.variables.items()}
    pads = {n: (p.data_ptr() // 4) % 4 for n, p in on.variables.items()}
    assert on.train(max_steps=3, log_every=1, save_summary_steps=1) == 3
    assert off.train(max_steps=3, log_every=1, save_summary_steps=0) == 3
    assert on.global_step == off.global_step == 3
    got, want = _state(on.train_step), _state(off.train_step)
    assert set(got) == set(want)
    differ = [k for k in want if not same_bits(got[k], want[k])]
    assert not differ, differ[:5]
    assert _events(ssd, tmp_path / "off") == ([], []) and not os.path.exists(tmp_path / "off" / "eval")
    assert off._hist_ring is None and off.train_step._hist_ring is None and off.train_step._hist_limits is None   # nothing enqueued or allocated

    events, files = _events(ssd, tmp_path / "on")
    assert len(files) == 1 and [step for _w, step, _v in events] == [1, 2, 3]
    log = [json.loads(l) for l in open(tmp_path / "on" / "train_log.jsonl")]
    assert [r["step"] for r in log] == [1, 2, 3]
    names = on.train_step.names
    for (_wall, step, values), record in zip(events, log):
        for tag, key in SCALAR_TAGS.items():
            assert values[tag] == float(f32(record[key])), (step, tag)
        assert ("global_step/sec" in values) == (step > 1)
        hist_tags = [t for t in values if t.endswith("_hist")]
        assert set(values) - set(hist_tags) - {"global_step/sec"} == set(SCALAR_TAGS) | set(MATCH_TAGS)
        per_level = [values[t] for t in MATCH_TAGS[:5]]
        # whole matches divided by the batch size 2; the levels add up to the total (small integers: exact in float32)
        assert all(v >= 0 and float(2 * v).is_integer() for v in per_level) and sum(per_level) == values[MATCH_TAGS[5]] >= 1.0
        assert all(n + "_hist" in values for n in names)
        grads = [n for n in names if n + "_grad_hist" in values]
        assert len(grads) >= len(names) - 20 and len(hist_tags) == len(names) + len(grads)
    assert events[1][2]["global_step/sec"] > 0

    # step 1: every variable's histogram is the restatement of the initial variable
    step1 = events[0][2]
    for n in names:
        h = step1[n + "_hist"]
        counts, st = ref.plane(initial[n].reshape(-1), pads[n])
        lim, bkt = ref.compressed(counts)
        assert h["num"] == float(st["num"]) == initial[n].size, n
        assert h["min"] == float(st["min"]) and h["max"] == float(st["max"]), n
        assert h["sum"] == float(st["sum"]) and h["sum_squares"] == float(st["sum_squares"]), n
        assert h["bucket_limit"] == lim and h["bucket"] == bkt, n
        g = step1.get(n + "_grad_hist")
        assert g is None or (g["num"] == initial[n].size and sum(g["bucket"]) == initial[n].size), n


def test_the_schedule_and_the_evaluation_directory(ssd, cuda, data, tmp_path):
    _premises(ssd, data)
    t = ssd.Trainer(_config(data, tmp_path / "run"), seed=SEED, read_workers=2)
    results = t.train_and_evaluate(max_steps=4, log_every=1, save_summary_steps=2)
    assert len(results) == 1 and results[0]["step"] == 4
    events, files = _events(ssd, tmp_path / "run")
    assert len(files) == 1 and [step for _w, step, _v in events] == [1, 3]
    evals, files = _events(ssd, tmp_path / "run" / "eval")
    assert len(files) == 1 and [step for _w, step, _v in evals] == [4]
    numeric = {k: v for k, v in results[0].items() if k != "step" and isinstance(v, (int, float)) and not isinstance(v, bool)}
    assert numeric and set(evals[0][2]) == set(numeric)
    for k, v in numeric.items():
        got = evals[0][2][k]
        assert got == float(f32(v)) or (np.isnan(got) and np.isnan(v)), k


def test_a_step_that_stops_the_run_writes_no_event(ssd, cuda, data, tmp_path):
    t = ssd.Trainer(_config(data, tmp_path / "run"), seed=SEED, read_workers=2)
    with cuda.no_grad():
        t.variables["box_net/encoded_boxes/bias"][5] = float("nan")
    with pytest.raises(FloatingPointError, match=r"step 1: variable 'box_net/encoded_boxes/bias' has 1 non-finite"):
        t.train(max_steps=3, log_every=1, save_summary_steps=1)
    events, _files = _events(ssd, tmp_path / "run")
    assert events == []
