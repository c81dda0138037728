"""The EVAL loss, host side (no GPU): the TFRecord reader, the loss config, the regularisation term, and the numpy
restatement of matching / targets / focal loss (tests/helpers/loss_ref.py) against hand-worked answers."""
import ctypes
import math
import os

import numpy as np
import pytest

import ssd_amd.evaluation  # noqa: F401  (a submodule the package does not import itself)
from helpers import example_protos, loss_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _examples(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        img = rng.integers(0, 256, (16 + 8 * i, 24, 3), dtype=np.uint8)
        k = int(rng.integers(0, 4))
        lo = rng.uniform(0.0, 0.45, (k, 2)).astype(np.float32)
        hi = lo + rng.uniform(0.1, 0.5, (k, 2)).astype(np.float32)
        boxes = np.concatenate([lo, hi], axis=1)[:, [0, 1, 2, 3]]
        labels = rng.integers(0, 80, k)
        out.append((example_protos.jpeg(img), boxes, labels))
    return out


@pytest.mark.parametrize("unpacked", [False, True])
def test_tfrecords_round_trip(ssd, tmp_path, unpacked):
    """Shards written with the official protobuf encoder, read back in train.py's sorted order (train.py:21-24)."""
    tfr = ssd.tfrecords
    shards = {"val-0001.tfrecords": _examples(3, 1), "val-0000.tfrecords": _examples(2, 2)}
    for name, exs in shards.items():
        tfr.write_records(str(tmp_path / name), [example_protos.example_bytes(j, b, l, unpacked=unpacked) for j, b, l in exs])
    (tmp_path / "notes.txt").write_text("not a shard")
    assert [os.path.basename(p) for p in tfr.shard_paths(str(tmp_path))] == ["val-0000.tfrecords", "val-0001.tfrecords"]
    got = list(tfr.read_dataset(str(tmp_path)))
    want = shards["val-0000.tfrecords"] + shards["val-0001.tfrecords"]
    assert len(got) == len(want)
    for (j, b, l), (wj, wb, wl) in zip(got, want):
        assert j == wj
        assert b.dtype == np.float32 and b.shape == (len(wl), 4) and np.array_equal(b, np.asarray(wb, np.float32).reshape(-1, 4))
        assert l.dtype == np.int32 and np.array_equal(l, wl)


def test_tfrecords_refuse_a_flipped_crc_byte(ssd, tmp_path):
    tfr = ssd.tfrecords
    path = str(tmp_path / "a.tfrecords")
    exs = _examples(2, 3)
    tfr.write_records(path, [example_protos.example_bytes(j, b, l) for j, b, l in exs])
    raw = bytearray(open(path, "rb").read())
    assert len(list(tfr.read_records(path))) == 2
    for pos, what in ((9, "length"), (len(raw) - 2, "record")):          # the length CRC of record 0, the data CRC of the last
        bad = bytearray(raw)
        bad[pos] ^= 0x01
        open(path, "wb").write(bytes(bad))
        with pytest.raises(ValueError, match="corrupt record"):
            list(tfr.read_records(path))
        assert len(list(tfr.read_records(path, verify=False))) == 2 or what == "length"
    bad = bytearray(raw)
    bad[20] ^= 0x40                                                       # a byte of record 0's payload
    open(path, "wb").write(bytes(bad))
    with pytest.raises(ValueError, match="CRC mismatch"):
        list(tfr.read_records(path))


def test_load_loss_config_on_the_reference_configs(ssd):
    for name in ("reference_config_mobilenet.json", "reference_config_shufflenet.json"):
        c = ssd.load_loss_config(os.path.join(HERE, "golden", name))
        assert c == {"gamma": 2.0, "alpha": 0.25, "localization_loss_weight": 1.0, "classification_loss_weight": 2.0,
                     "weight_decay": 5e-5}
    with pytest.raises(KeyError, match="gamma"):
        ssd.load_loss_config(os.path.join(HERE, "golden", "config_mobilenet.json"))      # an inference-only config
    # the inference surface is untouched
    assert ssd.load_config(os.path.join(HERE, "golden", "reference_config_mobilenet.json"))["num_classes"] == 80


def test_regularization_on_a_hand_computed_dict(ssd):
    W = {"a/weights": np.array([1.0, 2.0], np.float32), "b/kernel": np.array([[3.0]], np.float32),
         "c/depthwise_weights": np.array([10.0], np.float32), "d/gamma": np.array([100.0], np.float32),
         "e/biases": np.array([5.0], np.float32)}
    # l2_loss = sum(K^2) / 2: (1 + 4) / 2 + 9 / 2 = 7
    assert ssd.evaluation.l2_sum(W) == 7.0
    r = ssd.evaluation.regularization_loss(W, 0.5)
    assert r.dtype == np.float32 and r == np.float32(3.5)
    assert ssd.evaluation.regularization_loss(W, 5e-5) == np.float32(5e-5 * 7.0)


def test_total_loss_and_per_image_normaliser(ssd):
    lc = {"localization_loss_weight": 1.0, "classification_loss_weight": 2.0}
    loc, cls, tot = ssd.evaluation.image_losses(np.array([3.0, 5.0, 4.0], np.float32), np.float32(0.25),
                                                dict(lc, gamma=2.0, alpha=0.25, weight_decay=0.0))
    assert (loc, cls) == (np.float32(0.75), np.float32(1.25)) and tot == np.float32(0.75 + 2.5 + 0.25)
    loc, cls, _ = ssd.evaluation.image_losses(np.array([3.0, 5.0, 0.0], np.float32), np.float32(0), dict(lc, gamma=2, alpha=0.25))
    assert (loc, cls) == (np.float32(3.0), np.float32(5.0))              # max(matches, 1)


# ----------------------------------------------------------------------------- the restatement, hand-worked
def test_restatement_tie_takes_the_first_gt():
    anchors = np.array([[0, 0, 1, 1], [0, 0, 0.5, 0.5]], np.float32)
    gt = np.array([[0, 0, 1, 1], [0, 0, 1, 1]], np.float32)               # duplicate gt: IoU 1 with anchor 0 for both
    reg, cls, m = loss_ref.training_targets(anchors, gt, [7, 3])
    assert m.tolist() == [0, -1] and cls.tolist() == [8, 0]
    assert np.array_equal(reg, np.zeros((2, 4), np.float32))             # gt == anchor: every code 0 (log 1 = 0)


def test_restatement_forced_collision_with_a_masked_first_row():
    """gt 0 (IoU 0.0025 < 0.1: masked) and gt 1 (IoU 0.25) both pick anchor 0: the row id comes from the UNMASKED one-hot
    (gt 0), the mask from gt 1 -- anchor 0 is matched to gt 0 (training_target_creation.py:105-118, reproduced)."""
    anchors = np.array([[0, 0, 1, 1], [5, 5, 6, 6]], np.float32)
    gt = np.array([[0, 0, 0.05, 0.05], [0, 0, 0.5, 0.5]], np.float32)
    _reg, cls, m = loss_ref.training_targets(anchors, gt, [4, 9])
    assert m.tolist() == [0, -1] and cls.tolist() == [5, 0]


def test_restatement_all_zero_iou_gt_is_never_forced():
    anchors = np.array([[0, 0, 0.5, 0.5], [0.5, 0.5, 1, 1]], np.float32)
    gt = np.array([[0.5, 0.5, 1, 1], [3, 3, 4, 4]], np.float32)           # gt 1 overlaps nothing: picks anchor 0, masked
    _reg, cls, m = loss_ref.training_targets(anchors, gt, [0, 1])
    assert m.tolist() == [-1, 0] and cls.tolist() == [0, 1]


def test_restatement_no_gt():
    anchors = np.array([[0, 0, 0.5, 0.5], [0.5, 0.5, 1, 1]], np.float32)
    reg, cls, m = loss_ref.training_targets(anchors, np.zeros((0, 4), np.float32), [])
    assert m.tolist() == [-1, -1] and cls.tolist() == [0, 0] and not reg.any()


def test_restatement_ignore_between_thresholds():
    gt = np.array([[0, 0, 1, 1]], np.float32)
    anchors = np.array([[0, 0, 1, 0.45], [0, 0, 1, 0.3], [0, 0, 1, 1]], np.float32)   # IoU 0.45, 0.3, 1
    assert loss_ref.training_targets(anchors, gt, [2], pos=0.5, neg=0.4)[2].tolist() == [-2, -1, 0]
    assert loss_ref.training_targets(anchors, gt, [2], pos=0.5, neg=0.5)[2].tolist() == [-1, -1, 0]


def test_restatement_focal_and_smooth_l1_known_answers():
    # x = 0, background: -log p_t = ln 2, p_t = 1/2, (1 - p_t)^2 = 1/4, weight 1 - alpha = 3/4
    t = loss_ref.focal_terms(np.zeros((1, 2), np.float32), np.array([2]))
    assert t[0, 0] == np.float32(0.1875 * math.log(2.0))
    assert t[0, 1] == np.float32(np.float32(0.25) * np.float32(np.float32(0.25) * np.float32(math.log(2.0))))   # target: alpha
    assert loss_ref.smooth_l1(np.array([[0.5, 2.0, -1.0, 0.0]], np.float32), np.zeros((1, 4), np.float32)).tolist() == \
        [[0.125, 1.5, 0.5, 0.0]]
    # an ignored anchor (-2) contributes no classification loss, a negative one no localisation loss
    gt = np.array([[0, 0, 1, 1]], np.float32)
    anchors = np.array([[0, 0, 1, 0.45], [0, 0, 1, 0.3], [0, 0, 1, 1]], np.float32)
    cl, ll, m = loss_ref.image_losses(np.zeros((3, 2), np.float32), np.ones((3, 4), np.float32), anchors, gt, [0], pos=0.5, neg=0.4)
    assert m.tolist() == [-2, -1, 0] and cl[0] == 0 and cl[1] > 0 and ll[:2].tolist() == [0, 0] and ll[2] == np.float32(2.0)


def test_loss_entry_points_refuse_bad_arguments_without_a_gpu(ssd):
    """ssd_training_targets / ssd_loss check their arguments before any HIP call (include/ssd_hip.h conventions)."""
    L = ssd.lib()
    cfg = ssd.ssd._loss_config(0.5, 0.5)
    assert L.ssd_training_targets(None, 10, None, None, None, 1, 1, ctypes.byref(cfg), None, None, None, None, 0, None) < 0
    assert b"ssd_training_targets" in L.ssd_last_error()
    assert L.ssd_loss(None, None, None, 1, 10, 80, None, None, None, 1, ctypes.byref(cfg), None, None, None, None, None, 0, None) < 0
    assert b"ssd_loss" in L.ssd_last_error()
    assert L.ssd_loss_workspace_bytes(0, 10, 1) == 0 and L.ssd_loss_workspace_bytes(2, 100, 3) >= 2 * 3 * 8 + 2 * 2 * 48
    assert ctypes.sizeof(cfg) == 88                                         # ssd_loss_config's C layout
