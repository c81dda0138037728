"""-m gpu: ssd_voc_match and ssd_voc_curve (include/ssd_hip.h, "the VOC-style metric") against their numpy restatement bit for bit
and against coco_eval.Evaluator: the rows, the results, the dict, the host fallback of an oversize cell, cell and label lists longer
than one grid pass, every output element between guard words, streams, evaluation.evaluate end to end and the Trainer's evaluation."""
import numpy as np
import pytest

import ssd_amd.evaluation  # noqa: F401  (a submodule the package does not import itself)
from helpers import example_protos, guarded
from helpers import voc_match_cases as cases
from helpers import voc_match_ref as ref
from helpers.voc_match_cases import feed, rows_per_label, same_metrics

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


@pytest.fixture(scope="module")
def sets(ssd):
    """seed -> (images, Evaluator.evaluate()'s dict, the packed arrays, the restatement's (results, tp, tp_iou))"""
    out = {}
    for seed in cases.SEEDS:
        images = cases.make(seed)
        p = ssd.voc_match.pack(cases.NUM_CLASSES, *feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images)._flat())
        out[seed] = (images, feed(ssd.coco_eval.Evaluator(cases.NUM_CLASSES), images).evaluate(cases.THR), p,
                     ref.evaluate_packed(p, cases.THR, want_rows=True))
    return out


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_rows_and_results_equal_the_restatement_bit_for_bit(cuda, ssd, sets, seed):
    images, want, p, (r_res, r_tp, r_iou) = sets[seed]
    res, tp, tp_iou = ssd.voc_match.evaluate_packed(p, cases.THR, 0, want_rows=True)
    assert np.array_equal(tp, r_tp) and tp.sum() > 20
    assert np.array_equal(tp_iou.view(np.uint64), r_iou.view(np.uint64))
    for name in ssd.voc_match.RESULT_DTYPE.names:
        assert np.array_equal(bits(res[name]), bits(r_res[name])), (name, res[name], r_res[name])
    assert res.dtype == ssd.voc_match.RESULT_DTYPE and (res["reserved"] == 0).all()
    # ... and the dict against the Evaluator, on a device given as an index and as a torch.device
    for device in (0, cuda.device("cuda", 0)):
        got = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR, device=device)
        same_metrics(got, want, rows_per_label(images, cases.NUM_CLASSES))


def test_the_fallback_cell_is_placed(cuda, ssd, sets):
    images, want, p, _ = sets[1]
    (rows, dbox, gbox), = p["fallback"]
    assert len(gbox) == ssd.voc_match.MAX_GT + 1 and not np.isin(rows, p["det_pos"]).any()
    _res, tp, tp_iou = ssd.voc_match.evaluate_packed(p, cases.THR, 0, want_rows=True)
    assert tp[rows].tolist() == [1, 1, 0, 0] and tp_iou[rows].tolist() == [1.0, 1.0, 0.0, 0.0]
    # without it the label loses these two true positives
    less = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images[:-1]).evaluate(cases.THR, device=0)
    full = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR, device=0)
    true_positives = lambda m, run: rows_per_label(run, cases.NUM_CLASSES)[0] - m[0]["total_FP"]
    assert true_positives(full, images) == true_positives(less, images[:-1]) + 2 and full[0]["total_FN"] == want[0]["total_FN"]


def test_more_cells_than_one_grid_pass(cuda, ssd):
    vm = ssd.voc_match
    images = cases.one_per_cell(vm.GRID_CAP * vm.CELLS_PER_BLOCK + 2 * vm.CELLS_PER_BLOCK + 3)
    ev = feed(vm.VocEvaluator(1), images)
    p = vm.pack(1, *ev._flat())
    assert len(p["cells"]) == len(images) and (p["cells"]["D"] == 1).all() and (p["cells"]["G"] == 1).all()
    want = feed(ssd.coco_eval.Evaluator(1), images).evaluate()
    same_metrics(ev.evaluate(device=0), want, [len(images)])
    assert 0 < want[0]["total_FP"] < len(images)
    res, tp, tp_iou = vm.evaluate_packed(p, 0.5, 0, want_rows=True)
    r_res, r_tp, r_iou = ref.evaluate_packed(p, 0.5, want_rows=True)
    assert np.array_equal(tp, r_tp) and np.array_equal(tp_iou.view(np.uint64), r_iou.view(np.uint64)) and bits(res).tolist() == bits(r_res).tolist()


def test_more_labels_than_one_grid_pass(cuda, ssd):
    vm = ssd.voc_match
    n_labels = vm.GRID_CAP * vm.CELLS_PER_BLOCK + vm.CELLS_PER_BLOCK + 2
    images = cases.many_labels(n_labels)
    want = feed(ssd.coco_eval.Evaluator(n_labels), images).evaluate()
    got = feed(vm.VocEvaluator(n_labels), images).evaluate(device=0)
    same_metrics(got, want, rows_per_label(images, n_labels))
    assert [got[l]["AP"] for l in (0, 1, n_labels - 2, n_labels - 1)] == [float((l % 3) == 0) for l in (0, 1, n_labels - 2, n_labels - 1)]


@pytest.mark.parametrize("layout", ["skewed", "aligned"])
def test_every_output_is_written_between_guard_words(cuda, ssd, layout):
    """Both calls on tensors of ONE arena, every buffer between guard words; `skewed` puts every base at 16 (mod 32).  The outputs are
    prefilled with 0xFF bytes; no cell is oversize here, so det_pos is a permutation and every element of tp, tp_iou and the results
    must be written: the restatement, run over 0xFF-filled arrays as well, leaves no 0xFF byte pattern of its own."""
    vm = ssd.voc_match
    images = cases.make(0, oversize=False)
    p = vm.pack(cases.NUM_CLASSES, *feed(vm.VocEvaluator(cases.NUM_CLASSES), images)._flat())
    n, nd, ng, L = p["n_rows"], len(p["det_pos"]), len(p["gt_box"]), len(p["segments"])
    assert nd == n and not p["fallback"] and (p["cells"]["G"] == 0).any() and p["cells"]["G"].max() > 128 and (p["segments"]["count"] == 0).any()
    want_tp, want_iou = np.full(n, 0xFF, np.uint8), np.full(n, 0xFF, np.uint8).repeat(8).view(np.float64)
    ref.match(p["cells"], p["det_box"], p["det_pos"], p["gt_box"], cases.THR, want_tp, want_iou)
    want_res = ref.curve(p["segments"], want_tp, want_iou, p["conf"], vm.RESULT_DTYPE)
    assert want_tp.max() == 1 and not np.isnan(want_iou).any()
    arena = guarded.Arena(cuda, cuda.device("cuda", 0), layout)
    for k in ("cells", "segments", "det_box", "det_pos", "gt_box", "conf"):
        arena.add(k, bits(p[k]), np.uint8, 16, "input")
    arena.add("tp", (n,), np.uint8, 16, "output", fill=0xFF)
    arena.add("tp_iou", (n * 8,), np.uint8, 16, "output", fill=0xFF)
    arena.add("results", (L * 64,), np.uint8, 16, "output", fill=0xFF)
    v = arena.view
    if layout == "skewed":
        assert all(v(k).data_ptr() % 32 == 16 for k in arena.tensors)
    vm.launch(p["cells"], v("cells"), v("det_box"), v("det_pos"), nd, v("gt_box"), ng, cases.THR, v("tp"), v("tp_iou"), n,
              p["segments"], v("segments"), v("conf"), v("results"))
    cuda.cuda.synchronize()
    arena.check()
    out = arena.outputs()
    assert np.array_equal(out["tp"], want_tp)
    assert np.array_equal(out["tp_iou"], bits(want_iou))
    assert np.array_equal(out["results"], bits(want_res))


def test_a_side_stream_and_a_second_launch_give_the_same_bits(cuda, ssd, sets):
    images, want, p, _ = sets[2]
    vm = ssd.voc_match
    first = vm.evaluate_packed(p, cases.THR, 0, want_rows=True)
    second = vm.evaluate_packed(p, cases.THR, 0, want_rows=True)
    side = cuda.cuda.Stream(device=0)
    with cuda.cuda.stream(side):
        third = vm.evaluate_packed(p, cases.THR, 0, want_rows=True)
        got = feed(vm.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR, device=0)
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    same_metrics(got, want, rows_per_label(images, cases.NUM_CLASSES))
    timings = {}
    feed(vm.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR, device=0, timings=timings)
    assert set(timings) == {"pack", "upload", "match", "curve", "download", "dict"} and all(t >= 0 for t in timings.values())


def test_evaluation_module_with_the_gpu_metric(ssd, cuda, tmp_path, monkeypatch):
    """evaluation.evaluate on the synthetic shard of tests/test_gpu_loss.py's evaluation test, with and without metric_device: every
    key equal, 'metrics/mAP' equal or the adjacent float32 (the AP sums are formed in another order)."""
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 3, "score_threshold": 0.15, "iou_threshold": 0.6,
              "max_boxes_per_class": 25, "min_dimension": 128}
    config = dict(params, gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0, weight_decay=5e-5)
    W = ssd.synthetic_weights(params, seed=9, logits_bias=-1.0)
    rng = np.random.default_rng(4)
    records = []
    for h, w in [(128, 128), (100, 150), (160, 120), (128, 256), (90, 200), (200, 130), (128, 128)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        n = int(rng.integers(0, 4))
        lo = rng.uniform(0.0, 0.5, (n, 2))
        hi = lo + rng.uniform(0.1, 0.5, (n, 2))
        boxes = np.clip(np.concatenate([lo, hi], 1), 0, 1).astype(np.float32)
        records.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, n)))
    ssd.tfrecords.write_records(str(tmp_path / "val-00000.tfrecords"), records)
    seen = []
    inner = ssd.voc_match.VocEvaluator.evaluate

    def counting(self, *a, **kw):
        seen.append(sum(len(im[4]) for im in self.images))
        return inner(self, *a, **kw)
    monkeypatch.setattr(ssd.voc_match.VocEvaluator, "evaluate", counting)
    det = ssd.Detector(W, config=config)
    host = ssd.evaluation.evaluate(det, str(tmp_path), config, max_batch=4)
    gpu = ssd.evaluation.evaluate(det, str(tmp_path), config, max_batch=4, metric_device=0)
    det.close()
    assert seen and seen[0] > 0 and list(gpu) == list(host) and host["num_images"] == 7
    for k in host:
        if k != "metrics/mAP":
            assert gpu[k] == host[k], (k, gpu[k], host[k])
    a, b = np.float32(gpu["metrics/mAP"]), np.float32(host["metrics/mAP"])
    assert a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(-np.inf)), (a, b)


def test_the_trainer_passes_metric_device_on(ssd, cuda, tmp_path, monkeypatch):
    """Trainer(metric_device=0).evaluate() calls evaluation.evaluate with it, and its dict is the host metric's but for the mAP's last bit."""
    import os
    from conftest import TINY_PARAMS
    from ssd_amd import ckpt_export, evaluation
    rng = np.random.default_rng(7)
    for name, n in (("train", 4), ("val", 4)):
        recs = []
        for _ in range(n):
            img = rng.integers(0, 256, (int(rng.integers(90, 200)), int(rng.integers(90, 200)), 3), dtype=np.uint8)
            m = int(rng.integers(1, 4))
            c = rng.uniform(0.1, 0.6, (m, 2))
            boxes = np.concatenate([c, c + rng.uniform(0.15, 0.35, (m, 2))], 1).clip(0, 1)
            recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, m)))
        os.makedirs(str(tmp_path / name))
        ssd.tfrecords.write_records(str(tmp_path / name / (name + "-00.tfrecords")), recs)
    W = ssd.synthetic_weights(TINY_PARAMS, seed=301, logits_bias=-1.0)
    pretrained = ckpt_export.write_checkpoint(str(tmp_path / "pretrained.ckpt"), {k: v for k, v in W.items() if k.startswith("MobilenetV1/")})
    cfg = dict(TINY_PARAMS, batch_size=2, image_height=128, image_width=128, initial_learning_rate=1e-3, num_steps=100, weight_decay=1e-4,
               gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0, model_dir=str(tmp_path / "run"),
               train_dataset=str(tmp_path / "train"), val_dataset=str(tmp_path / "val"), pretrained_checkpoint=pretrained)
    seen, inner = [], evaluation.evaluate

    def recording(*a, **kw):
        seen.append(kw.get("metric_device"))
        return inner(*a, **kw)
    monkeypatch.setattr(evaluation, "evaluate", recording)
    t = ssd.Trainer(cfg, read_workers=2, metric_device=0)
    res = t.evaluate()
    assert seen == [0] and res["num_images"] == 4
    with ssd.Detector(cfg["model_dir"], config=cfg, use_ema=True) as det:
        host = inner(det, cfg["val_dataset"], cfg, read_workers=2)
    assert list(res) == list(host) + ["step"]
    for k in host:
        if k != "metrics/mAP":
            assert res[k] == host[k], (k, res[k], host[k])
    a, b = np.float32(res["metrics/mAP"]), np.float32(host["metrics/mAP"])
    assert a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(-np.inf)), (a, b)
