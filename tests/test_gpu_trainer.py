"""ssd_amd.Trainer on the GPU: a resumed run continues bit for bit and follows the documented sequence,
train_and_evaluate writes its logs and evaluates the moving averages, a non-finite variable stops the run before any checkpoint, and
one ShuffleNet step runs and is saved.  TINY_PARAMS at 128 x 128, batch 2, on a 24-record shard (test_gpu_train_from_pipeline.py's
writer, restated) and a 4-image validation shard."""
import json
import os

import numpy as np
import pytest

from helpers import example_protos
from helpers.head_train_gpu import same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
# The run's seed.  40 is a seed -- found on the CPU through host_batches -- for which every image of the first three batches
# of the pipelines started at global_step 0 and at global_step 2 keeps a box (two batches are used, a third is prefetched); asserted
# in _premises.
SEED = 40
BASE = dict(TINY_PARAMS, batch_size=2, image_height=128, image_width=128, initial_learning_rate=1e-3, num_steps=100, weight_decay=1e-4,
            gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0)
SCOPES = {"mobilenet": "MobilenetV1/", "shufflenet": "ShuffleNetV2/"}


def _write_shard(directory, name, n, seed):
    """n JPEGs of random sizes with 1 .. 3 boxes each."""
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
    """The shards and one pretrained checkpoint per backbone: the backbone subset of synthetic_weights plus a classifier's variable."""
    from ssd_amd import ckpt_export
    root = tmp_path_factory.mktemp("trainer")
    out = {"train_dataset": _write_shard(str(root / "train"), "train-00.tfrecords", 24, 0),
           "val_dataset": _write_shard(str(root / "val"), "val-00.tfrecords", 4, 1)}
    for backbone, scope in SCOPES.items():
        W = ssd.synthetic_weights(dict(TINY_PARAMS, backbone=backbone), seed=301, logits_bias=-4.0)
        ckpt = {k: v for k, v in W.items() if k.startswith(scope)}
        ckpt[scope + "Logits/weights"] = np.ones((1, 1, 4, 10), f32)
        out[backbone] = ckpt_export.write_checkpoint(str(root / (backbone + "_pretrained.ckpt")), ckpt)
    return out


def _config(data, model_dir, backbone="mobilenet"):
    return dict(BASE, backbone=backbone, model_dir=str(model_dir), train_dataset=data["train_dataset"], val_dataset=data["val_dataset"],
                pretrained_checkpoint=data[backbone])


def _premises(ssd, data, starts):
    """On the CPU: every image of the first three batches of the pipeline started at each of `starts` keeps a box."""
    from ssd_amd.trainer import pipeline_seed
    for start in starts:
        host = ssd.TrainPipeline(data["train_dataset"], BASE, seed=pipeline_seed(SEED, start), read_workers=2).host_batches()
        for _ in range(3):
            kept = [len(labels) for _frame, _row, _boxes, labels in next(host)]
            assert len(kept) == 2 and min(kept) >= 1, (start, kept)
        host.close()


def _state(ts):
    """Every variable, moving statistic, average and both slots of a TrainStep as host arrays."""
    out = {"statistic " + n: s.detach().cpu().numpy() for n, s in ts.statistics.items()}
    for n in ts.names:
        m, v = ts.slots(n)
        out.update({"variable " + n: ts.parameters[n].detach().cpu().numpy(), "average " + n: ts.ema(n).cpu().numpy(),
                    "m " + n: m.cpu().numpy(), "v " + n: v.cpu().numpy()})
    return out


def test_resume_is_lossless_and_the_sequence_is_the_documented_one(ssd, cuda, data, tmp_path):
    from ssd_amd import trainer
    _premises(ssd, data, (0, 2))
    cfg = _config(data, tmp_path / "run")
    a = ssd.Trainer(cfg, seed=SEED, read_workers=2)
    assert a.resumed_from is None and a.global_step == 0
    assert a.train(max_steps=2, log_every=1) == 2
    assert ssd.resolve_checkpoint(cfg["model_dir"]).endswith("model.ckpt-2")
    del a
    b = ssd.Trainer(cfg, seed=SEED, read_workers=2)
    assert b.resumed_from.endswith("model.ckpt-2") and b.global_step == 2
    assert b.train(max_steps=4, log_every=1) == 4
    got = _state(b.train_step)

    # the same four steps by hand: no save, no restore, no norms()
    W = {**trainer.warm_start_weights(data["mobilenet"], TINY_PARAMS), **trainer.head_tower_weights(TINY_PARAMS, SEED)}
    backbone = ssd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", seed=SEED, train_first=True).train()
    fpn = ssd.TrainableFPN(TINY_PARAMS, W, device="cuda", seed=SEED).train()
    head = ssd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda", seed=SEED).train()
    variables = {**backbone.named_variables(), **fpn.named_variables(), **head.named_variables()}
    statistics = {**backbone.statistics(), **fpn.statistics(), **head.statistics()}
    ts = ssd.TrainStep(variables, cfg, statistics, layout="tf", params=TINY_PARAMS, frozen={})
    anchors = cuda.from_numpy(ssd.AnchorGenerator()(128, 128)).cuda()
    for start in (0, 2):
        pipe = ssd.TrainPipeline(data["train_dataset"], cfg, seed=trainer.pipeline_seed(SEED, start), read_workers=2)
        for _ in range(2):
            images, gt = next(pipe)
            for p in variables.values():
                p.grad = None
            eb, cp = head(fpn(backbone(images)))
            out = ssd.differentiable_loss(cp, eb, anchors, gt, cfg)
            loss = float(f32(cfg["localization_loss_weight"])) * out["localization_loss"] \
                + float(f32(cfg["classification_loss_weight"])) * out["classification_loss"]
            loss.backward()
            ts.step()
        pipe._gen.close()
    assert ts.global_step == 4 == b.train_step.global_step
    want = _state(ts)
    assert set(got) == set(want) and len(want) == 4 * len(ts.names) + len(statistics)
    differ = [k for k in want if not same_bits(got[k], want[k])]
    assert not differ, differ[:5]
    for n in ("MobilenetV1/Conv2d_0/weights", "MobilenetV1/Conv2d_13_pointwise/weights"):     # the warm-started backbone was trained
        assert not same_bits(want["variable " + n], W[n]), n
    # the log holds the four steps, written by the two runs
    steps = [json.loads(l)["step"] for l in open(os.path.join(cfg["model_dir"], "train_log.jsonl"))]
    assert steps == [1, 2, 3, 4]


def test_train_and_evaluate_logs_and_evaluates_the_moving_averages(ssd, cuda, data, tmp_path):
    from ssd_amd import evaluation
    _premises(ssd, data, (0,))
    cfg = _config(data, tmp_path / "run")
    t = ssd.Trainer(cfg, seed=SEED, read_workers=2)
    start = {n: p.detach().cpu().numpy().copy() for n, p in t.variables.items()}
    results = t.train_and_evaluate(max_steps=2, eval_every_steps=1, log_every=1)
    evals = [json.loads(l) for l in open(os.path.join(cfg["model_dir"], "eval_log.jsonl"))]
    assert [e["step"] for e in evals] == [1, 2] and evals == results
    with ssd.Detector(cfg["model_dir"], config=cfg, use_ema=True) as det:
        direct = evaluation.evaluate(det, cfg["val_dataset"], cfg, read_workers=2)
    assert evals[-1] == dict(direct, step=2) and direct["num_images"] == 4
    log = [json.loads(l) for l in open(os.path.join(cfg["model_dir"], "train_log.jsonl"))]
    assert [r["step"] for r in log] == [1, 2]
    for r in log:
        assert all(np.isfinite(v) for v in r.values()), r
        assert r["localization_loss"] > 0 and r["classification_loss"] > 0 and r["gradient_norm"] > 0 and r["images_per_second"] > 0
        assert r["loss"] == float(evaluation.total_loss(f32(r["localization_loss"]), f32(r["classification_loss"]),
                                                        f32(r["regularization_loss"]), cfg))
    assert log[0]["learning_rate"] == 1e-3 and 0 < log[1]["learning_rate"] < 1e-3
    reg = f32(log[0]["regularization_loss"])
    ref = evaluation.regularization_loss(start, cfg["weight_decay"])
    print("step 1 regularization_loss: trainer %r, evaluation %r" % (float(reg), float(ref)))
    assert reg == ref or reg in (np.nextafter(ref, f32(np.inf)), np.nextafter(ref, f32(-np.inf)))
    assert ssd.resolve_checkpoint(cfg["model_dir"]).endswith("model.ckpt-2")
    assert 'model_checkpoint_path: "model.ckpt-2"' in open(os.path.join(cfg["model_dir"], "checkpoint")).read()


def test_a_non_finite_variable_stops_the_run_before_any_checkpoint(ssd, cuda, data, tmp_path):
    from ssd_amd import trainer
    cfg = _config(data, tmp_path / "run")
    t = ssd.Trainer(cfg, seed=SEED, read_workers=2)
    with cuda.no_grad():
        t.variables["box_net/encoded_boxes/bias"][5] = float("nan")
    with pytest.raises(FloatingPointError, match=r"step 1: variable 'box_net/encoded_boxes/bias' has 1 non-finite"):
        t.train(max_steps=3, log_every=1)
    assert trainer.checkpoint_steps(cfg["model_dir"]) == []
    assert not [f for f in os.listdir(cfg["model_dir"]) if f.startswith(("model.ckpt", "checkpoint"))]
    with pytest.raises(RuntimeError, match="non-finite"):
        t.save()


def test_one_shufflenet_step_is_finite_and_saved(ssd, cuda, data, tmp_path):
    _premises(ssd, data, (0,))
    cfg = _config(data, tmp_path / "run", "shufflenet")
    t = ssd.Trainer(cfg, seed=SEED, read_workers=2)
    assert t.train(max_steps=1, log_every=1) == 1
    (r,) = [json.loads(l) for l in open(os.path.join(cfg["model_dir"], "train_log.jsonl"))]
    assert r["step"] == 1 and all(np.isfinite(v) for v in r.values()) and r["loss"] > 0 and r["gradient_norm"] > 0
    prefix = ssd.resolve_checkpoint(cfg["model_dir"])
    assert prefix.endswith("model.ckpt-1")
    saved = ssd.read_checkpoint(prefix, ["global_step", "ShuffleNetV2/Conv1/weights"])
    assert int(saved["global_step"]) == 1
    assert same_bits(saved["ShuffleNetV2/Conv1/weights"], t.variables["ShuffleNetV2/Conv1/weights"].detach().cpu().numpy())
