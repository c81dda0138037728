"""The Trainer's host logic without a GPU: load_run_config, the warm start from a pretrained checkpoint, the schedules, the pipeline
seed, checkpoint pruning and the stop-on-non-finite decision."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MOBILENET = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15, "iou_threshold": 0.6,
             "max_boxes_per_class": 25}
SHUFFLENET = dict(MOBILENET, backbone="shufflenet")


def test_load_run_config(ssd):
    keys = ("model_dir", "train_dataset", "val_dataset", "pretrained_checkpoint")
    assert ssd.RUN_KEYS == keys
    cfg = {k: "/somewhere/" + k for k in keys}
    assert ssd.load_run_config(dict(cfg, backbone="mobilenet")) == cfg
    for k in keys:
        with pytest.raises(KeyError, match=k):
            ssd.load_run_config({q: v for q, v in cfg.items() if q != k})
    for name in ("reference_config_mobilenet.json", "reference_config_shufflenet.json"):
        got = ssd.load_run_config(os.path.join(HERE, "golden", name))
        assert tuple(got) == keys and all(isinstance(v, str) and v for v in got.values())
        assert "ckpt" in got["pretrained_checkpoint"] and got["model_dir"].startswith("models/")


@pytest.mark.parametrize("params,scope,extra", [(MOBILENET, "MobilenetV1/", "MobilenetV1/Logits/Conv2d_1c_1x1/weights"),
                                                (SHUFFLENET, "ShuffleNetV2/", "ShuffleNetV2/classifier/weights")],
                         ids=["mobilenet", "shufflenet"])
def test_warm_start_reads_exactly_the_backbone(ssd, tmp_path, params, scope, extra):
    from ssd_amd import ckpt_export, trainer
    W = ssd.synthetic_weights(params, seed=11)
    backbone = {k: v for k, v in W.items() if k.startswith(scope)}
    assert 0 < len(backbone) < len(W) and set(backbone) == set(trainer.backbone_names(params))
    first = next(iter(backbone))
    ckpt = dict(backbone)
    ckpt[extra] = np.ones((1, 1, 8, 1001), np.float32)                          # a classifier's head: ignored
    ckpt[first + "/Adam"] = np.zeros_like(backbone[first])                       # a slot variable: ignored
    ckpt[first + "/ExponentialMovingAverage"] = backbone[first] + 1              # an average: ignored (the raw variable is read)
    ckpt["global_step"] = np.int64(1000)
    prefix = ckpt_export.write_checkpoint(str(tmp_path / "pretrained.ckpt"), ckpt)
    got = trainer.warm_start_weights(prefix, params)
    assert set(got) == set(backbone)
    for k, v in backbone.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v), k
    assert trainer.warm_start_weights(prefix + ".index", params).keys() == got.keys()
    # a missing backbone variable is named
    victim = sorted(backbone)[len(backbone) // 2]
    short = {k: v for k, v in ckpt.items() if k != victim}
    p2 = ckpt_export.write_checkpoint(str(tmp_path / "short.ckpt"), short)
    with pytest.raises(KeyError, match=victim):
        trainer.warm_start_weights(p2, params)
    # a wrong shape
    bad = dict(ckpt)
    bad[victim] = np.zeros(tuple(backbone[victim].shape) + (2,), np.float32)
    p3 = ckpt_export.write_checkpoint(str(tmp_path / "shape.ckpt"), bad)
    with pytest.raises(ValueError, match="shape"):
        trainer.warm_start_weights(p3, params)
    with pytest.raises(FileNotFoundError):
        trainer.warm_start_weights(str(tmp_path / "nothing.ckpt"), params)


def test_head_tower_weights_complete_the_warm_start(ssd):
    from ssd_amd import trainer
    shapes = ssd.head_variable_shapes(MOBILENET)
    a, b, c = (trainer.head_tower_weights(MOBILENET, s) for s in (0, 0, 1))
    assert set(a) == {k for k in shapes if not k.startswith("class_net/logits/")}
    for k, v in a.items():
        assert v.dtype == np.float32 and tuple(v.shape) == tuple(shapes[k]) and np.array_equal(v, b[k]), k
    k = "box_net/conv3x3_0/kernel"
    assert not np.array_equal(a[k], c[k])
    s = np.sqrt(1.0 / (9 * 256)) / 0.87962566103423978
    assert np.abs(a[k]).max() <= 2 * s and abs(float(a[k].std()) - np.sqrt(1.0 / (9 * 256))) < 0.02 * s
    assert not a["box_net/encoded_boxes/bias"].any() and abs(float(a["box_net/encoded_boxes/kernel"].std()) - 0.01) < 5e-4
    assert (a["class_net/batch_norm_2_for_level_5/gamma"] == 1).all() and (a["class_net/batch_norm_2_for_level_5/moving_variance"] == 1).all()
    assert not a["class_net/batch_norm_2_for_level_5/beta"].any() and not a["class_net/batch_norm_2_for_level_5/moving_mean"].any()


def test_due_on_step_and_time_schedules(ssd):
    from ssd_amd.trainer import due
    # steps: every 3 after the last at 4
    assert [s for s in range(4, 12) if due(s, 0.0, 4, 0.0, 3, None)] == [7, 8, 9, 10, 11]
    assert not due(4, 1e9, 4, 0.0, 1, 1.0)                                       # never twice for one step
    assert due(5, 0.0, 4, 0.0, 1, None) and not due(5, 0.0, 4, 0.0, 2, None)
    # time: 1800 s after the last
    assert not due(5, 1799.9, 4, 0.0, None, 1800) and due(5, 1800.0, 4, 0.0, None, 1800)
    assert not due(5, 2800.0, 4, 1000.1, None, 1800) and due(5, 2800.2, 4, 1000.1, None, 1800)
    # the step schedule wins when both are given; neither: never
    assert not due(5, 1e9, 4, 0.0, 10, 1.0) and due(14, 0.0, 4, 0.0, 10, 1e9)
    assert not due(100, 1e9, 0, 0.0, None, None)


def test_pipeline_seed_differs_per_start_step_and_is_stable(ssd):
    from ssd_amd.trainer import pipeline_seed

    def draws(seq):
        return np.random.default_rng(np.random.SeedSequence(seq)).integers(0, 2 ** 62, 4).tolist()
    seen = {tuple(draws(pipeline_seed(seed, step))) for seed in (0, 1, 7) for step in (0, 1, 2, 1000)}
    assert len(seen) == 12
    assert pipeline_seed(3, 5) == [3, 5] and draws(pipeline_seed(3, 5)) == draws(pipeline_seed(3, 5)) == draws([3, 5])
    assert draws(pipeline_seed(3, 5)) != draws(pipeline_seed(5, 3))
    # TrainPipeline spawns its two generators from it
    a, b = np.random.SeedSequence(pipeline_seed(3, 5)).spawn(2)
    assert np.random.default_rng(a).integers(0, 2 ** 62) != np.random.default_rng(b).integers(0, 2 ** 62)
    with pytest.raises(ValueError):
        pipeline_seed(-1, 0)


def test_prune_checkpoints_keeps_the_newest_five_and_the_state_file_resolves(ssd, tmp_path):
    from ssd_amd import ckpt_export, trainer
    d = str(tmp_path)
    steps = [2, 10, 9, 100, 30, 31, 7, 1000]                                     # not in order, and "100" < "30" as strings
    for s in steps:
        ckpt_export.write_checkpoint(os.path.join(d, "model.ckpt-%d" % s), {"global_step": np.int64(s), "x": np.full(3, s, np.float32)})
    ckpt_export.write_checkpoint_state(d, "model.ckpt-1000")
    open(os.path.join(d, "train_log.jsonl"), "w").write("{}\n")
    assert trainer.checkpoint_steps(d) == sorted(steps)
    removed = trainer.prune_checkpoints(d, 5)
    assert [os.path.basename(p) for p in removed] == ["model.ckpt-2", "model.ckpt-7", "model.ckpt-9"]
    assert trainer.checkpoint_steps(d) == [10, 30, 31, 100, 1000]
    left = sorted(os.listdir(d))
    assert "checkpoint" in left and "train_log.jsonl" in left and not any(f.startswith(("model.ckpt-2.", "model.ckpt-7.", "model.ckpt-9.")) for f in left)
    assert len([f for f in left if f.startswith("model.ckpt-")]) == 10           # an index and a data file each
    assert ssd.resolve_checkpoint(d) == os.path.join(d, "model.ckpt-1000")
    assert int(ssd.read_checkpoint(ssd.resolve_checkpoint(d), ["global_step"])["global_step"]) == 1000
    assert trainer.prune_checkpoints(d, 5) == [] and trainer.prune_checkpoints(str(tmp_path / "none"), 5) == []
    with pytest.raises(ValueError):
        trainer.prune_checkpoints(d, 0)


def test_the_non_finite_decision_names_the_step_and_the_first_bad_variable(ssd):
    from ssd_amd.trainer import first_non_finite
    names = ["a/weights", "b/gamma", "c/bias", "d/kernel"]
    sums = np.ones((4, 2))
    bad = np.zeros((4, 2), np.int64)
    assert first_non_finite(7, names, 1.0, 2.0, sums, bad) is None
    b = bad.copy()
    b[2, 0], b[3, 1] = 3, 1
    msg = first_non_finite(7, names, float("nan"), 2.0, sums, b)
    assert msg.startswith("step 7:") and "variable 'c/bias'" in msg and "3 non-finite" in msg and "d/kernel" not in msg
    b[0, 1] = 5                                                                 # an earlier row's gradient: the variable still comes first
    assert "variable 'c/bias'" in first_non_finite(7, names, 1.0, 2.0, sums, b)
    b = bad.copy()
    b[1, 1] = 2
    msg = first_non_finite(8, names, 1.0, 2.0, sums, b)
    assert msg.startswith("step 8:") and "gradient of 'b/gamma'" in msg
    s = sums.copy()
    s[3, 1] = np.inf                                                            # finite elements whose squares overflow the sum
    msg = first_non_finite(9, names, 1.0, 2.0, s, bad)
    assert msg.startswith("step 9:") and "d/kernel" in msg and "sum of squares" in msg
    assert "localization_loss" in first_non_finite(3, names, float("inf"), 2.0, sums, bad)
    msg = first_non_finite(3, names, 1.0, float("nan"), sums, bad)
    assert msg.startswith("step 3:") and "classification_loss" in msg


def test_log_record_uses_total_loss_and_the_gradient_norm(ssd):
    from ssd_amd import evaluation
    from ssd_amd.trainer import log_record
    lc = {"localization_loss_weight": 1.0, "classification_loss_weight": 2.0}
    sums = np.array([[4.0, 9.0], [1.0, 16.0]])
    r = log_record(5, np.float32(0.3), np.float32(0.7), np.float32(0.05), sums, lc, 1e-3, 12.5, 0.25)
    assert r["step"] == 5 and r["gradient_norm"] == 5.0 and r["learning_rate"] == 1e-3 and r["images_per_second"] == 12.5
    assert r["loss"] == float(evaluation.total_loss(np.float32(0.3), np.float32(0.7), np.float32(0.05), lc))
    assert r["regularization_loss"] == float(np.float32(0.05)) and r["wait_seconds"] == 0.25
