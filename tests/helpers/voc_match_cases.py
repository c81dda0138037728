"""The VOC-style metric's test set (include/ssd_hip.h, "the VOC-style metric"): a few hundred small random images of 5 classes plus
three crafted ones, and counters of the situations the kernels must get right -- the tests assert each counter positive on every
seed, so a changed generator cannot quietly stop covering one.

Every corner lies on a 4-pixel grid and every confidence is a float32 twentieth, so equal IoUs, IoUs of exactly 0.5 and equal
confidences across images actually occur.  Random part: an image is empty with probability 0.1; else 0 to 4 groundtruth boxes of
labels 0..3 (a box is duplicated with probability 0.25), per box of labels 0..2 up to 2 detections that copy it (shifted by a grid
step with probability 0.6), and up to 2 stray detections of labels 0, 1, 2, 4.  Label 3 never has detections, label 4 never has
groundtruth.  Crafted: image A -- an IoU of exactly 0.5, a second detection of a taken box, a duplicated box detected twice; image B
-- a cell of 72 and a cell of 130 groundtruth boxes with equal boxes in one lane's column and across lanes; image C (oversize=True)
-- a cell of MAX_GT + 1 boxes."""
import collections

import numpy as np

SEEDS = (0, 1, 2)
NUM_CLASSES = 5
THR = 0.5
COUNTERS = ("IoU tie inside a cell", "IoU equals the threshold", "second detection of a taken box",
            "detections on an image without groundtruth of the label", "equal confidences in different images of a label",
            "labels without detections", "labels without groundtruth", "images without any box", "cells over 64 groundtruth boxes",
            "cells over 128 groundtruth boxes", "cells over MAX_GT", "labels whose rows exceed 64 and are no multiple of 64")


EXACT = ("precision", "recall", "best_threshold", "mean_iou_for_TP", "total_FP", "total_FN")


def same_metrics(got, want, rows):
    """rows[label]: the label's detections.  The six values == and of the same type; AP within 2 * tp * 2^-53: both are sums of tp
    non-negative terms that total at most 1 (the recall steps, each times a precision <= 1), and each order's error is at most
    gamma(tp - 1) <= tp * 2^-53 of that total.  mAP: the mean of such values, off by at most the mean of their bounds plus its own
    roundings.  -> the worst |AP - host AP| / bound"""
    num_classes = len(rows)
    assert list(got) == list(want)
    worst, slack = 0.0, 0.0
    for label in range(num_classes):
        g, w = got[label], want[label]
        assert list(g) == list(w)
        for k in EXACT:
            assert type(g[k]) is type(w[k]) and g[k] == w[k], (label, k, g[k], w[k])
        bound = 2.0 * (rows[label] - w["total_FP"]) * 2.0 ** -53
        assert type(g["AP"]) is float and abs(g["AP"] - w["AP"]) <= bound, (label, g["AP"], w["AP"], bound)
        worst = max(worst, abs(g["AP"] - w["AP"]) / bound if bound else 0.0)
        slack += bound
    if num_classes > 1:
        assert type(got["mAP"]) is float and abs(got["mAP"] - want["mAP"]) <= slack / num_classes + 2.0 ** -51
    return worst


def feed(evaluator, images):
    for im in images:
        evaluator.add_image(*im)
    return evaluator


def rows_per_label(images, num_classes):
    return np.bincount(np.concatenate([im[3] for im in images]), minlength=num_classes).tolist()


def _image(gt, dets):
    """[(box, label)], [(box, label, score)] -> add_image's five arrays"""
    return (np.array([g[0] for g in gt], np.float64).reshape(-1, 4), np.array([g[1] for g in gt], np.int64),
            np.array([d[0] for d in dets], np.float32).reshape(-1, 4), np.array([d[1] for d in dets], np.int64),
            np.array([d[2] for d in dets], np.float32))


def _grid_boxes(n, per_row, side):
    k = np.arange(n)
    y, x = side * (k // per_row), side * (k % per_row)
    return np.stack([y, x, y + side, x + side], 1).astype(np.float64)


def make(seed, n_img=150, oversize=True, max_gt=4096):
    """-> the images of a run: a list of (gt_boxes, gt_labels, boxes, labels, scores)"""
    rng = np.random.default_rng(seed)
    score = lambda: np.float32(int(rng.integers(3, 20)) / 20.0)
    images = []
    for _ in range(n_img):
        gt, dets = [], []
        if rng.random() >= 0.1:
            for _g in range(int(rng.integers(0, 5))):
                y, x = 4 * rng.integers(0, 16, 2)
                h, w = 4 * rng.integers(2, 12, 2)
                box, label = [int(y), int(x), int(y + h), int(x + w)], int(rng.integers(0, 4))
                gt.append((box, label))
                if rng.random() < 0.25:
                    gt.append((list(box), label))
                for _d in range(int(rng.integers(0, 3)) if label < 3 else 0):
                    j = 4 * rng.integers(-1, 2, 4) * (rng.random() < 0.6)
                    b = [box[0] + int(j[0]), box[1] + int(j[1]), box[2] + int(j[2]), box[3] + int(j[3])]
                    dets.append((b, label, score()))
            for _d in range(int(rng.integers(0, 3))):
                y, x = 4 * rng.integers(0, 16, 2)
                s = 4 * int(rng.integers(2, 12))
                dets.append(([int(y), int(x), int(y) + s, int(x) + s], int(rng.choice([0, 1, 2, 4])), score()))
        images.append(_image(gt, dets))
    # image A, label 0
    dup = [40, 40, 60, 60]
    images.append(_image([([0, 0, 8, 16], 0), (dup, 0), (list(dup), 0)],
                         [([0, 0, 8, 8], 0, 0.9), ([0, 0, 8, 16], 0, 0.8), (dup, 0, 0.85), (dup, 0, 0.85), (dup, 0, 0.3)]))
    # image B: 72 boxes of label 1 (box 67 = box 3: one lane's column; box 70 = box 5: across lanes), 130 of label 2
    b1, b2 = _grid_boxes(72, 16, 8), _grid_boxes(130, 16, 8)
    b1[67], b1[70] = b1[3], b1[5]
    b2[129], b2[128] = b2[1], b2[64]
    gt = [(b.tolist(), 1) for b in b1] + [(b.tolist(), 2) for b in b2]
    dets = []
    for label, boxes, picks in ((1, b1, (3, 3, 5, 5, 69, 66, 0, 65)), (2, b2, (1, 1, 64, 64, 129, 127, 100, 63))):
        for n, k in enumerate(picks):
            dets.append((boxes[k].tolist(), label, np.float32((19 - n) / 20.0)))
        y0, x0, y1, x1 = boxes[10]
        dets.append(([y0, x0 + 4, y1, x1 + 4], label, np.float32(0.5)))           # IoU 1/3 with two neighbours: a tie below the threshold
        dets.append(([y0, x0, y1, x1 + 4], label, np.float32(0.45)))              # IoU 2/3 with box 10
    images.append(_image(gt, dets))
    if oversize:
        big = _grid_boxes(max_gt + 1, 64, 4)
        images.append(_image([(b, 0) for b in big.tolist()] + [([0, 0, 8, 8], 1)],
                             [(big[max_gt].tolist(), 0, 0.95), (big[0].tolist(), 0, 0.7), (big[0].tolist(), 0, 0.65),
                              ([0, 0, 4, 8], 0, 0.6), ([0, 0, 8, 8], 1, 0.55)]))
    return images


def one_per_cell(n):
    """n images with one box and one detection of label 0 each: n cells"""
    images = []
    for k in range(n):
        box = [0, 0, 8 + 4 * (k % 5), 8]
        images.append(_image([(box, 0)], [([0, 0, 8 + 4 * (k % 3), 8], 0, np.float32((1 + k % 19) / 20.0))]))
    return images


def many_labels(n_labels):
    """four detections of four labels per image, every label once; every third label has a matching box"""
    images = []
    for first in range(0, n_labels, 4):
        labels = list(range(first, min(first + 4, n_labels)))
        box = [4, 4, 20, 24]
        images.append(_image([(box, l) for l in labels if l % 3 == 0], [(box, l, np.float32((1 + l % 19) / 20.0)) for l in labels]))
    return images


def counts(images, num_classes, thr, iou_matrix, max_gt=4096):
    """The situations of COUNTERS in `images`, counted by a plain walk in Evaluator's order (iou_matrix: coco_eval._iou_matrix)."""
    cnt = collections.Counter()
    rows = collections.defaultdict(list)                               # label -> [(conf, image, box)]
    gts = collections.defaultdict(list)                                # (label, image) -> [box]
    n_gt = collections.Counter()
    for img, (gb, gl, b, l, s) in enumerate(images):
        if len(gl) == 0 and len(l) == 0:
            cnt["images without any box"] += 1
        for box, label in zip(gb, gl.tolist()):
            gts[(label, img)].append(box)
            n_gt[label] += 1
        for box, label, conf in zip(np.asarray(b, np.float64), l.tolist(), s.tolist()):
            rows[label].append((conf, img, box))
    for key, boxes in gts.items():
        cnt["cells over 64 groundtruth boxes"] += 64 < len(boxes) <= max_gt
        cnt["cells over 128 groundtruth boxes"] += 128 < len(boxes) <= max_gt
        cnt["cells over MAX_GT"] += len(boxes) > max_gt
    for label in range(num_classes):
        det = rows[label]
        cnt["labels without detections"] += not det
        cnt["labels without groundtruth"] += n_gt[label] == 0
        cnt["labels whose rows exceed 64 and are no multiple of 64"] += len(det) > 64 and len(det) % 64 != 0
        by_conf = collections.defaultdict(set)
        for conf, img, _box in det:
            by_conf[conf].add(img)
        cnt["equal confidences in different images of a label"] += sum(len(v) > 1 for v in by_conf.values())
        taken = {}
        for conf, img, box in sorted(det, key=lambda r: -r[0]):
            g = gts.get((label, img))
            if not g:
                cnt["detections on an image without groundtruth of the label"] += 1
                continue
            iou = iou_matrix(box[None], np.array(g, np.float64))[0]
            best = int(np.argmax(iou))
            cnt["IoU tie inside a cell"] += iou[best] > 0 and np.count_nonzero(iou == iou[best]) > 1
            cnt["IoU equals the threshold"] += iou[best] == thr
            if iou[best] > 0 and iou[best] >= thr:
                if taken.get((img, best)):
                    cnt["second detection of a taken box"] += 1
                taken[(img, best)] = True
    return cnt
