"""Record blocks for the COCO rows (include/ssd_hip.h, "the COCO rows"), shared by tests/test_coco_rows_host.py and
tests/test_gpu_coco_rows.py, and the dict route they are measured against.

A case is a dict: records int32 [n, 6T + 1], image_ids (ascending), image_hw [n, 2], mapping {label: category id}, cat_ids
(ascending), thr.  MAPPING sends 7 labels to 5 categories in non-monotone order, two labels to one category and one label (2) to a
category that is not evaluated."""
import numpy as np

MAPPING = {0: 40, 1: 10, 2: 99, 3: 50, 4: 20, 5: 30, 6: 10}
CAT_IDS = [10, 20, 30, 40, 50]
SIZES = [(480, 640), (500, 375), (333, 500), (427, 640), (612, 612), (375, 500), (640, 480), (97, 203), (128, 128), (300, 128),
         (1, 1), (1200, 1600)]
WIDTHS = (640, 500, 427, 375, 333, 480, 612)


def split(rec):
    """boxes [n, T, 4] f32, labels [n, T] i32, scores [n, T] f32, num_boxes [n] i32 as views (ssd.split_records, restated)"""
    n, words = rec.shape
    T = (words - 1) // 6
    return rec[:, :4 * T].view(np.float32).reshape(n, T, 4), rec[:, 5 * T:6 * T], rec[:, 4 * T:5 * T].view(np.float32), rec[:, 6 * T]


def label_to_cat(case):
    out = np.full(max(case["mapping"]) + 1, -1, np.int32)
    for label, cat in case["mapping"].items():
        out[label] = case["cat_ids"].index(cat) if cat in case["cat_ids"] else -1
    return out


def _case(rec, hw, thr=0.15, first_id=100):
    return {"records": rec, "image_ids": [first_id + 7 * k for k in range(len(rec))], "image_hw": np.array(hw, np.int32).reshape(-1, 2),
            "mapping": dict(MAPPING), "cat_ids": list(CAT_IDS), "thr": thr}


def random_case(seed, T=24):
    """12 images of different sizes; image 3 has num_boxes 0, image 5 num_boxes T; scores from a few float32 values (ties); behind
    num_boxes NaN boxes, scores of 9.0 and labels no mapping has."""
    rng = np.random.default_rng(seed)
    n = len(SIZES)
    rec = np.zeros((n, 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    lo = rng.random((n, T, 2), dtype=np.float32) * np.float32(0.8)
    boxes[:, :, :2] = lo
    boxes[:, :, 2:] = np.minimum(lo + rng.random((n, T, 2), dtype=np.float32) * np.float32(0.6), np.float32(1.0))
    labels[:] = rng.integers(0, 7, (n, T))
    scores[:] = rng.choice(np.array([0.05, 0.15, 0.150001, 0.2, 0.35, 0.35, 0.5, 0.75, 0.9], np.float32), (n, T))
    num[:] = rng.integers(1, T, n)
    num[3], num[5] = 0, T
    for i in range(n):
        boxes[i, num[i]:] = np.nan
        scores[i, num[i]:] = 9.0
        labels[i, num[i]:] = 1 << 20
    return _case(rec, SIZES)


def threshold_case(thr=0.15):
    """scores exactly float32(thr), one ulp above and one below, beside clear ones"""
    t = np.float32(thr)
    s = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.9, 0.01, t, np.nextafter(t, np.float32(1)), 0.5], np.float32)
    T = len(s)
    rec = np.zeros((2, 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    boxes[:] = np.array([0.1, 0.2, 0.7, 0.9], np.float32)
    labels[:] = [1, 1, 1, 4, 4, 6, 6, 0]
    scores[:] = s
    num[:] = [T, T - 1]
    return _case(rec, [(480, 640), (333, 500)], thr)


def truncation_case():
    """T = 256: image 0 has 130 rows of category 10 (labels 1 and 6) whose equal scores straddle rank 100, image 1 exactly 100,
    image 2 exactly 101; a few rows of other categories between them"""
    T = 256
    rec = np.zeros((3, 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    rng = np.random.default_rng(5)
    boxes[:, :, :2] = rng.random((3, T, 2), dtype=np.float32) * np.float32(0.5)
    boxes[:, :, 2:] = boxes[:, :, :2] + np.float32(0.25)
    for i, rows in enumerate((130, 100, 101)):
        labels[i, :rows] = np.where(np.arange(rows) % 3 == 0, 6, 1)
        labels[i, rows:rows + 9] = [0, 3, 4, 5, 2, 0, 3, 4, 5]
        num[i] = rows + 9
        scores[i, :] = 0.9
        # 90 distinct scores above, then 40 / 10 / 11 rows of ONE score: ranks 90 .. 129 tie, the record row decides who stays
        scores[i, :90] = (np.float32(0.3) + rng.permutation(90).astype(np.float32) / np.float32(256))
        scores[i, 90:rows] = np.float32(0.25)
    return _case(rec, [(480, 640), (500, 375), (640, 480)])


def contraction_boxes(draws=2_000_000):
    """A stream of COCO-like boxes: float32 xmin uniform in [0, 1), xmax = min(xmin + 0.5 * u, 1), a width from WIDTHS.  -> (xmin, xmax, W, w
    unfused, kind) of the draws whose w = trunc(fl32(xmax * W - xmin * W)) changes when hipcc's contraction fuses the SECOND product
    into the subtraction (kind 2: fl32(xmax * W exact - fl32(xmin * W))) or the FIRST (kind 1).  The products of a float32 and a
    small integer and their differences are exact in float64, so float64 arithmetic rounded once to float32 is the fused result."""
    rng = np.random.default_rng(0)
    xmin = rng.random(draws, dtype=np.float32)
    xmax = np.minimum(xmin + np.float32(0.5) * rng.random(draws, dtype=np.float32), np.float32(1.0))
    W = rng.choice(np.array(WIDTHS, np.int32), draws)
    Wf = W.astype(np.float32)
    a, b = xmin * Wf, xmax * Wf                                           # float32 products, each rounded
    a64, b64 = xmin.astype(np.float64) * W, xmax.astype(np.float64) * W   # exact
    plain = np.trunc(b - a)
    fused2 = np.trunc((b64 - a.astype(np.float64)).astype(np.float32))
    fused1 = np.trunc((b.astype(np.float64) - a64).astype(np.float32))
    kind = np.where(fused2 != plain, 2, 0) | np.where(fused1 != plain, 1, 0)
    at = np.nonzero(kind)[0]
    return xmin[at], xmax[at], W[at], plain[at].astype(np.int64), kind[at]


def contraction_case():
    """One image per width (height = width) holding that width's contraction-sensitive boxes, the same pair as y and as x
    -> the case and the unfused (w, kind) per image in record order"""
    xmin, xmax, W, w, kind = contraction_boxes()
    per = [np.nonzero(W == width)[0] for width in WIDTHS]
    T = max(8, max(len(p) for p in per))
    rec = np.zeros((len(WIDTHS), 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    want = []
    for i, p in enumerate(per):
        boxes[i, :len(p)] = np.stack([xmin[p], xmin[p], xmax[p], xmax[p]], axis=1)
        labels[i, :len(p)] = 4
        scores[i, :len(p)] = np.float32(0.9) - np.arange(len(p), dtype=np.float32) / np.float32(1024)      # record order = rank
        num[i] = len(p)
        want.append((w[p], kind[p]))
    return _case(rec, [(width, width) for width in WIDTHS]), want


def from_results(gt, dets, T=256, side=256):
    """A tests/helpers/coco_match_cases set as records: every image `side` square (a power of two: box / side and its products are
    exact), category c is label c - 1, the detections of an image in list order.  -> (annotations with the sizes, records, image ids,
    mapping, the result list with its scores rounded to float32, as a record holds them)"""
    ids = sorted(im["id"] for im in gt["images"])
    rec = np.zeros((len(ids), 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    at = {i: k for k, i in enumerate(ids)}
    for d in dets:
        i = at[d["image_id"]]
        x, y, w, h = d["bbox"]
        boxes[i, num[i]] = [y / side, x / side, (y + h) / side, (x + w) / side]
        labels[i, num[i]] = d["category_id"] - 1
        scores[i, num[i]] = d["score"]
        num[i] += 1
    sized = dict(gt, images=[dict(im, height=side, width=side) for im in gt["images"]])
    mapping = {c["id"] - 1: c["id"] for c in gt["categories"]}
    return sized, rec, ids, mapping, [dict(d, score=float(np.float32(d["score"]))) for d in dets]


def dict_route(ssd, case):
    """score_filter -> detection_records -> CocoBoxEval -> coco_match.pack for a case -> pack()'s dict"""
    results = []
    for i, (h, w), b, l, s, n in zip(case["image_ids"], case["image_hw"].tolist(), *split(case["records"])):
        results += ssd.coco_eval.detection_records(None, np.empty((h, w, 0), np.uint8), i, case["mapping"], case["thr"],
                                                   detections=ssd.ssd.score_filter(b, l, s, n, case["thr"]))
    gt = {"images": [{"id": i} for i in case["image_ids"]], "annotations": [], "categories": [{"id": c} for c in case["cat_ids"]]}
    ev = ssd.coco_metric.CocoBoxEval(gt, results)
    return ssd.coco_match.pack(ev._gts, ev._dts, ev.cat_ids, ev.img_ids)


def as_pack(rows, case):
    """rows_host / rows_device output -> keys and cells of coco_match.pack for a run without groundtruth"""
    counts = np.asarray(rows["counts"])
    K, n = counts.shape
    flat = counts.reshape(-1).astype(np.int64)
    at = np.nonzero(flat)[0]
    keys = [(case["cat_ids"][c // n], case["image_ids"][c % n]) for c in at.tolist()]
    return keys, flat[at], (np.cumsum(flat) - flat)[at]
