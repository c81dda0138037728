"""The EVAL loss on the GPU (loss.hip: ssd_training_targets, ssd_loss) against the float32 numpy restatement
(tests/helpers/loss_ref.py) and a float64 evaluation; SSD.loss, Detector.loss and the evaluation module end to end."""
import ctypes

import numpy as np
import pytest

import ssd_amd.evaluation  # noqa: F401  (a submodule the package does not import itself)
from helpers import example_protos, loss_ref

pytestmark = pytest.mark.gpu


def _gt_batch(anchors, counts, seed):
    """[B,G,4] boxes near random anchors (a mix of IoUs), with a duplicate gt and a gt equal to an anchor in every image
    that has room for them; labels in [0, 80)."""
    rng = np.random.default_rng(seed)
    B, G = len(counts), max(max(counts), 1)
    boxes = np.zeros((B, G, 4), np.float32)
    labels = rng.integers(0, 80, (B, G)).astype(np.int32)
    for b, n in enumerate(counts):
        idx = rng.integers(0, len(anchors), n)
        a = anchors[idx].astype(np.float64)
        h, w = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cy = (a[:, 0] + a[:, 2]) / 2 + rng.normal(0, 0.15, n) * h
        cx = (a[:, 1] + a[:, 3]) / 2 + rng.normal(0, 0.15, n) * w
        h = h * np.exp(rng.normal(0, 0.3, n))
        w = w * np.exp(rng.normal(0, 0.3, n))
        boxes[b, :n] = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(np.float32)
        if n >= 3:
            boxes[b, 1] = boxes[b, 0]                       # duplicate gt
            boxes[b, 2] = anchors[idx[2]]                   # gt == an anchor
    return boxes, labels, np.array(counts, np.int32)


def _ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("hw", [(640, 896), (128, 128), (384, 256)])
def test_training_targets_against_restatement(ssd, cuda, hw):
    anchors = ssd.AnchorGenerator()(*hw)
    boxes, labels, num = _gt_batch(anchors, [0, 1, 7, 100, 300], seed=hw[0] + hw[1])
    a_dev = cuda.from_numpy(anchors).cuda()
    reg, cls, m = (t.cpu().numpy() for t in ssd.get_training_targets(a_dev, boxes, labels, num))
    for b in range(len(num)):
        n = int(num[b])
        r_reg, r_cls, r_m = loss_ref.training_targets(anchors, boxes[b, :n], labels[b, :n])
        assert np.array_equal(m[b], r_m), (hw, n, np.flatnonzero(m[b] != r_m)[:10])
        assert np.array_equal(cls[b], r_cls)
        assert np.array_equal(reg[b][:, :2], r_reg[:, :2])               # ty, tx: one fp32 op each
        assert _ulp_diff(reg[b][:, 2:], r_reg[:, 2:]).max() <= 1          # th, tw: log correctly rounded on both sides
        if n >= 1:
            assert (m[b] >= 0).sum() >= 1
    # pos != neg: the ignore band (-2) exists on the GPU too
    _, _, m2 = ssd.get_training_targets(a_dev, boxes, labels, num, positives_threshold=0.5, negatives_threshold=0.3)
    m2 = m2.cpu().numpy()
    r = loss_ref.training_targets(anchors, boxes[4, :300], labels[4, :300], pos=0.5, neg=0.3)[2]
    assert np.array_equal(m2[4], r) and (r == -2).any()


def _loss_inputs(ssd, cuda, hw, C, counts, seed):
    g = ssd.AnchorGenerator()
    anchors = g(*hw)
    rng = np.random.default_rng(seed)
    B, N = len(counts), len(anchors)
    logits = rng.normal(-3.0, 2.0, (B, N, C)).astype(np.float32)
    codes = rng.normal(0.0, 1.5, (B, N, 4)).astype(np.float32)
    boxes, labels, num = _gt_batch(anchors, counts, seed)
    labels %= C
    return g, anchors, logits, codes, boxes, labels, num


@pytest.mark.parametrize("C", [80, 7])
def test_loss_against_restatement_and_float64(ssd, cuda, C):
    g, anchors, logits, codes, boxes, labels, num = _loss_inputs(ssd, cuda, (256, 384), C, [0, 1, 7, 100, 300], seed=C)
    dev = [cuda.from_numpy(x).cuda() for x in (logits, codes, anchors)]
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    levels = g.num_anchors_per_feature_map
    losses, per, cl, ll = ssd.ssd_loss(*dev, gt, anchors_per_level=levels, per_anchor=True)
    losses, per, cl, ll = (t.cpu().numpy() for t in (losses, per, cl, ll))
    r_losses, r_per, r_cl, r_ll = loss_ref.batch_losses(logits, codes, anchors, boxes, labels, num)
    np.testing.assert_allclose(cl, r_cl, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ll, r_ll, rtol=1e-6, atol=0)
    np.testing.assert_allclose(per[:, :2], r_per[:, :2], rtol=1e-6)
    assert np.array_equal(per[:, 2], r_per[:, 2])
    # matches per level
    for b in range(len(num)):
        m = loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]])[2]
        edges = np.cumsum([0] + list(levels))
        assert per[b, 3:].tolist() == [float((m[edges[k]:edges[k + 1]] >= 0).sum()) for k in range(len(levels))]
    f64 = loss_ref.losses_f64(logits, codes, anchors, boxes, labels, num)
    np.testing.assert_allclose(losses, f64, rtol=1e-5)
    np.testing.assert_allclose(losses, r_losses, rtol=1e-6)
    # two runs: the same bits
    again = ssd.ssd_loss(*dev, gt, anchors_per_level=levels, per_anchor=True)
    for x, y in zip((losses, per, cl, ll), again):
        assert np.array_equal(x, y.cpu().numpy())
    # the optional outputs are optional: no per-anchor and no per-image tensors
    L = ssd.lib()
    B, N = logits.shape[:2]
    bx, lb, nm = (cuda.from_numpy(np.ascontiguousarray(x)).cuda() for x in (boxes, labels, num))
    out = cuda.full((2,), -1.0, device="cuda")
    nbytes = L.ssd_loss_workspace_bytes(B, N, boxes.shape[1])
    ws = cuda.empty((nbytes,), dtype=cuda.uint8, device="cuda")
    cfg = ssd.ssd._loss_config(0.5, 0.5, 2.0, 0.25, ())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.ssd_loss(p(dev[0]), p(dev[1]), p(dev[2]), B, N, C, p(bx), p(lb), p(nm), boxes.shape[1], ctypes.byref(cfg),
                    None, p(out), None, None, p(ws), nbytes, None)
    assert rc == 0
    cuda.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), losses)
    assert L.ssd_loss(p(dev[0]), p(dev[1]), p(dev[2]), B, N, C, p(bx), p(lb), p(nm), boxes.shape[1], ctypes.byref(cfg),
                      None, p(out), None, None, p(ws), nbytes - 8, None) < 0             # workspace too small: refused
    assert L.ssd_loss_workspace_bytes(B, N, 5000) > 0
    assert L.ssd_loss(p(dev[0]), p(dev[1]), p(dev[2]), B, N, C, p(bx), p(lb), p(nm), 5000, ctypes.byref(cfg),
                      None, p(out), None, None, p(ws), 1 << 40, None) < 0               # G beyond SSD_LOSS_MAX_GT
    assert b"4096" in L.ssd_last_error()


def _params(backbone, num_classes=80):
    return {"backbone": backbone, "depth_multiplier": 1.0 if backbone == "mobilenet" else 0.5, "num_classes": num_classes,
            "score_threshold": 0.15, "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 128}


def _restated_ssd_loss(ssd, eng, anchors, boxes, labels, num):
    lg = eng.get_tensor("class_predictions")
    cd = eng.get_tensor("encoded_boxes")
    B = boxes.shape[0]
    return loss_ref.batch_losses(lg.reshape(B, len(anchors), -1), cd.reshape(B, len(anchors), 4), anchors, boxes, labels, num)


@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_ssd_loss_end_to_end(ssd, cuda, backbone):
    params = _params(backbone)
    W = ssd.synthetic_weights(params, seed=5, logits_bias=-2.5)
    eng = ssd.Engine(params, W, device=0, precision="f32")
    lp = {"gamma": 2.0, "alpha": 0.25}
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (3, 128, 256, 3), dtype=np.uint8)
    anchors = ssd.AnchorGenerator()(128, 256)
    boxes, labels, num = _gt_batch(anchors, [4, 0, 12], seed=3)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    x = cuda.from_numpy(imgs).cuda()
    model = ssd.SSD(x, eng)
    out = model.loss(gt, lp)
    got = np.array([out["localization_loss"].item(), out["classification_loss"].item()], np.float32)
    r_losses, r_per, _, _ = _restated_ssd_loss(ssd, eng, anchors, boxes, labels, num)      # B > 1: the batch's normaliser
    np.testing.assert_allclose(got, r_losses, rtol=1e-6)
    assert np.array_equal(model.matches_per_image.cpu().numpy(), r_per[:, 2])
    assert model.matches_per_level.shape == (3, 5)
    # two batches back to back on one stream == one at a time
    single = []
    for b in range(3):
        mb = ssd.SSD(x[b:b + 1], eng)
        o = mb.loss({"boxes": boxes[b:b + 1], "labels": labels[b:b + 1], "num_boxes": num[b:b + 1]}, lp)
        single.append((o["localization_loss"].item(), o["classification_loss"].item()))
    m1, m2 = ssd.SSD(x[0:1], eng), None
    o1 = m1.loss({"boxes": boxes[:1], "labels": labels[:1], "num_boxes": num[:1]}, lp)
    m2 = ssd.SSD(x[2:3], eng)
    o2 = m2.loss({"boxes": boxes[2:], "labels": labels[2:], "num_boxes": num[2:]}, lp)
    assert (o1["localization_loss"].item(), o1["classification_loss"].item()) == single[0]
    assert (o2["localization_loss"].item(), o2["classification_loss"].item()) == single[2]
    # a mixed-size batch (three source sizes, one network shape) gives every image's one-at-a-time values
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(100, 128, 3), (120, 160, 3), (128, 256, 3)]]
    gts = [(np.array([[0.1, 0.1, 0.6, 0.5], [0.3, 0.2, 0.9, 0.9]], np.float32), np.array([1, 5])),
           (np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)), (np.array([[0.0, 0.0, 1.0, 1.0]], np.float32), np.array([79]))]
    run = ssd.evaluation._Run(eng)
    lc = {"gamma": 2.0, "alpha": 0.25}
    mixed = run(frames, gts, lc)
    for f, gtb, res in zip(frames, gts, mixed):
        one = run([f], [gtb], lc)[0]
        assert np.array_equal(one[0], res[0])
        for u, v in zip(one[2], res[2]):
            assert np.array_equal(u, v)
    # mode f16x3 within 1e-4 of f32
    eng.set_precision("f16x3")
    o16 = ssd.SSD(x, eng).loss(gt, lp)
    assert eng.status() == 0
    np.testing.assert_allclose([o16["localization_loss"].item(), o16["classification_loss"].item()], got, rtol=1e-4)
    eng.close()


def test_evaluation_module_on_a_synthetic_shard(ssd, cuda, tmp_path):
    params = _params("mobilenet", num_classes=3)
    config = dict(params, gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0, weight_decay=5e-5)
    W = ssd.synthetic_weights(params, seed=9, logits_bias=-1.0)
    rng = np.random.default_rng(4)
    sizes = [(128, 128), (100, 150), (160, 120), (128, 256), (90, 200), (200, 130), (128, 128)]
    records, raw = [], []
    for k, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        n = int(rng.integers(0, 4))
        lo = rng.uniform(0.0, 0.5, (n, 2))
        hi = lo + rng.uniform(0.1, 0.5, (n, 2))
        boxes = np.clip(np.concatenate([lo, hi], 1), 0, 1).astype(np.float32)
        labels = rng.integers(0, 3, n)
        jp = example_protos.jpeg(img)
        records.append(example_protos.example_bytes(jp, boxes, labels))
        raw.append((jp, boxes, labels))
    shard = str(tmp_path / "val-00000.tfrecords")
    ssd.tfrecords.write_records(shard, records)
    det = ssd.Detector(W, config=config)
    res = ssd.evaluation.evaluate(det, str(tmp_path), config, max_batch=4)
    # loss = the mean over images of Detector.loss (batch 1, the image's own normaliser)
    import io
    from PIL import Image
    per, ev = [], ssd.coco_eval.Evaluator(3)
    for jp, boxes, labels in raw:
        img = np.asarray(Image.open(io.BytesIO(jp)).convert("RGB"), dtype=np.uint8)
        per.append(det.loss(img, boxes, labels))
        # the Evaluator by hand: predictions NOT divided by box_scaler, groundtruth multiplied by it
        x = cuda.from_numpy(img[None].copy()).cuda()
        m = ssd.SSD(x, det.engine)
        bx, sc, cl, nm = (t.cpu().numpy() for t in ssd.batch_multiclass_non_max_suppression(
            m.raw_predictions["encoded_boxes"], m.anchors, m.raw_predictions["class_predictions"], params["score_threshold"],
            params["iou_threshold"], params["max_boxes_per_class"], box_scaler=None))
        n = int(nm[0])
        ev.add_image(boxes * m.box_scaler, labels, bx[0, :n], cl[0, :n], sc[0, :n])
    assert res["num_images"] == len(sizes)
    for key in ("loss", "localization_loss", "classification_loss", "regularization_loss"):
        want = float(np.float32(np.mean([float(p[key]) for p in per])))
        assert res[key] == want, (key, res[key], want)
    assert per[0]["regularization_loss"] == ssd.evaluation.regularization_loss(W, 5e-5)
    assert res["metrics/mAP"] == float(np.float32(ev.evaluate()["mAP"]))
    assert any(p["classification_loss"] > 0 for p in per)
    det.close()
