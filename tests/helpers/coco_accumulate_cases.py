"""The COCO accumulation's test sets (include/ssd_hip.h, "the COCO accumulation").

hand_built(): one annotation file and result list whose categories are each the smallest shape at which the curve kernel can go
wrong; SHAPES names what every category is for, and the tests assert from the packed arrays that the shape is really there.
Groundtruth boxes sit on a grid of 40 x 40 boxes 50 apart (area 1600: regular at 'all' and 'medium', ignored at 'small' and
'large'); a detection is the box of groundtruth box (d mod G) shifted right by 0 .. 9 pixels (IoU 1 .. 0.63: matched at some
thresholds only, a second detection of a box unmatched), or a stray far from every box.  Scores come from a few float32 values, so
ties inside cells and across images are the rule.

flat(): random flat arrays for the entry point itself -- any T, A, K -- where the matching's words are random bits."""
import numpy as np

SCORES = [0.2, 0.35, 0.35, 0.5, 0.5, 0.5, 0.75, 0.9]
# category -> what it is for, {image: (groundtruth boxes, detections)}
SHAPES = {
    1: ("groundtruth but no detection", {1: (3, 0), 2: (2, 0)}),
    2: ("detections but no groundtruth", {1: (0, 4), 3: (0, 1)}),
    3: ("every box small: -1 at medium and large, a curve at all and small", {1: (4, 6), 2: (3, 5)}),
    4: ("scores tied across images and inside a cell", {1: (3, 8), 2: (3, 8), 3: (2, 8)}),
    5: ("a cell of 130 detections", {1: (2, 130), 2: (3, 7)}),
    6: ("ignored rows in front of the first true positive", {1: (3, 9), 2: (2, 3)}),
    7: ("npig 1", {2: (1, 5)}),
    8: ("npig 3", {1: (2, 4), 3: (1, 4)}),
    9: ("npig 100", {1: (100, 90), 2: (0, 12)}),
    10: ("npig 150", {1: (80, 70), 2: (70, 75)}),
    11: ("a segment of 1 row", {3: (2, 1)}),
    12: ("a segment of 63 rows", {1: (9, 30), 2: (9, 33)}),
    13: ("a segment of 64 rows", {1: (9, 30), 2: (9, 34)}),
    14: ("a segment of 65 rows", {1: (9, 30), 2: (9, 35)}),
    15: ("a segment of 128 rows", {1: (20, 60), 2: (20, 60), 3: (1, 8)}),
    16: ("a segment of 129 rows", {1: (20, 60), 2: (20, 60), 3: (1, 9)}),
}
N_IMAGES = 3
EMPTY_CATEGORY = 17                            # listed in the annotation file, no box and no detection: a segment with both counts 0


def hand_built(seed=7):
    """-> (annotation dict, result list)"""
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    for cat, (_what, cells) in SHAPES.items():
        side = 10 if cat == 3 else 40
        for img, (G, D) in cells.items():
            boxes = [[50 * (g % 10), 50 * (g // 10), side, side] for g in range(G)]
            for g, bb in enumerate(boxes):
                crowd = cat == 6 and img == 1 and g == 0
                anns.append({"image_id": img, "category_id": cat, "bbox": bb, "area": float(side * side), "iscrowd": int(crowd)})
            for d in range(D):
                score = float(np.float32(rng.choice(SCORES)))
                if G and rng.random() < 0.8:
                    b = boxes[d % G]
                    bb = [b[0] + int(rng.integers(0, 10 if side == 40 else 3)), b[1], side, side]
                else:
                    bb = [5000 + 50 * d, 5000, side, side]
                if cat == 6 and img == 1 and d < 4:             # the best detections all sit on the crowd box: ignored rows lead
                    bb, score = [d % 2, 0, side, side], float(np.float32(0.95))
                if cat == 6 and img == 2:                       # ... then true positives in the other image
                    bb, score = list(boxes[d % G]), float(np.float32(0.9))
                dets.append({"image_id": img, "category_id": cat, "bbox": bb, "score": score})
    gt = {"images": [{"id": i} for i in range(1, N_IMAGES + 1)], "annotations": anns, "categories": [{"id": c} for c in sorted(SHAPES)] + [{"id": EMPTY_CATEGORY}]}
    return gt, dets


def flat(seed, det_counts, gt_counts, T, A, segment_dtype, max_det=100):
    """Random flat arrays of the entry point: category k has det_counts[k] rows, in cells of 1 .. max_det rows, and gt_counts[k]
    groundtruth flags.  -> dict: segments, order int32, rank uint8, matched / ignored uint16 [A, nd], gt_ignore uint8 [A, ng], nd, ng.
    matched & ignored occurs (a detection matched to an ignored box), and so does ignored alone (unmatched, out of range)."""
    rng = np.random.default_rng(seed)
    det_counts, gt_counts = np.asarray(det_counts, np.int64), np.asarray(gt_counts, np.int64)
    K, nd, ng = len(det_counts), int(det_counts.sum()), int(gt_counts.sum())
    segments = np.zeros(K, segment_dtype)
    segments["det_count"], segments["gt_count"] = det_counts, gt_counts
    segments["det_begin"], segments["gt_begin"] = np.cumsum(det_counts) - det_counts, np.cumsum(gt_counts) - gt_counts
    rank = np.zeros(nd, np.uint8)
    score = np.zeros(nd)
    at = 0
    for n in det_counts.tolist():
        left = n
        while left:
            d = int(min(left, rng.integers(1, max_det + 1)))
            rank[at:at + d] = np.arange(d)
            score[at:at + d] = -np.sort(-rng.choice(SCORES, d))          # descending inside a cell
            at, left = at + d, left - d
    cat_of = np.repeat(np.arange(K), det_counts)
    order = np.lexsort((-score, cat_of)).astype(np.int32)
    full = (1 << T) - 1
    matched = rng.integers(0, full + 1, (A, nd)).astype(np.uint16)
    ignored = (rng.integers(0, full + 1, (A, nd)) & rng.integers(0, full + 1, (A, nd))).astype(np.uint16)
    gt_ignore = (rng.random((A, ng)) < 0.3).astype(np.uint8)
    return {"segments": segments, "order": order, "rank": rank, "matched": matched, "ignored": ignored, "gt_ignore": gt_ignore, "nd": nd, "ng": ng}
