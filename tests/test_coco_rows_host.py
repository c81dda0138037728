"""The COCO rows without a GPU (include/ssd_hip.h, "the COCO rows"): coco_rows.rows_host against the dict route -- score_filter,
detection_records, CocoBoxEval, coco_match.pack -- bit for bit; the threshold's edge, the truncation at 100, the boxes that a fused
multiply-add would change; write_predictions against json.dumps; the records the header calls bad; CocoBoxEval.from_records on the
host; the header's constants and the entry points' refusals, which come before any HIP call."""
import json
import os
import re

import numpy as np
import pytest

from helpers import coco_match_cases as cases
from helpers import coco_rows_cases as rcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = ("det_box", "det_area", "det_score")


def same_array(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def host_rows(ssd, case):
    return ssd.coco_rows.rows_host(case["records"], case["image_hw"], rcases.label_to_cat(case), len(case["cat_ids"]), case["thr"],
                                   image_ids=case["image_ids"])


def equals_dict_route(ssd, case):
    """keys, cells, det_box, det_area, det_score: equal in dtype, shape and bits -> the dict route's pack"""
    rows, want = host_rows(ssd, case), rcases.dict_route(ssd, case)
    keys, D, begin = rcases.as_pack(rows, case)
    assert rows["counts"].dtype == np.int32 and rows["counts"].shape == (len(case["cat_ids"]), len(case["image_ids"]))
    assert keys == want["keys"]
    assert np.array_equal(D, want["cells"]["D"]) and np.array_equal(begin, want["cells"]["det_begin"])
    for k in PACKED:
        assert same_array(rows[k], want[k]), k
    return rows, want


def test_python_constants_are_the_headers(ssd):
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    cr = ssd.coco_rows
    assert (cr.ROWS_MAX_T, cr.MAX_DET, cr.CELLS_PER_BLOCK, cr.GRID_CAP) == tuple(
        value("SSD_COCO_" + n) for n in ("ROWS_MAX_T", "MAX_DET", "CELLS_PER_BLOCK", "GRID_CAP"))
    assert float(cr.BOX_LIMIT) == 2.0 ** 30 and "below 2^30 in magnitude" in hdr
    # the reference's configs fit: T = num_classes * max_boxes_per_class
    for name in ("config_mobilenet.json", "config_shufflenet.json"):
        cfg = ssd.config.load_config(os.path.join(ROOT, "tests", "golden", name))
        assert cfg["num_classes"] * cfg["max_boxes_per_class"] <= cr.ROWS_MAX_T


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_rows_host_equals_the_dict_route(ssd, seed):
    case = rcases.random_case(seed)
    rows, want = equals_dict_route(ssd, case)
    counts = rows["counts"]
    assert (counts[:, 3] == 0).all() and counts[:, 5].sum() > 0 and (counts == 0).any() and (counts > 1).any()
    assert len(rows["det_score"]) > 50 and not (rows["det_score"] == 9.0).any() and np.isfinite(rows["det_box"]).all()
    # something of every kind was dropped: below the threshold, the label without a category
    boxes, labels, scores, num = rcases.split(case["records"])
    live = np.arange(scores.shape[1])[None, :] < num[:, None]
    assert (live & (scores <= np.float32(0.15))).any() and (live & (scores > np.float32(0.15)) & (labels == 2)).any()
    assert counts.sum() == (live & (scores > np.float32(0.15)) & (labels != 2)).sum()


def test_the_threshold_is_float32_and_strict(ssd):
    case = rcases.threshold_case()
    rows, _ = equals_dict_route(ssd, case)
    t = np.float32(0.15)
    up = np.nextafter(t, np.float32(1))
    # image 0: of category 10 (labels 1, 6) the ulp above twice; image 1 (num_boxes T - 1) loses nothing of it
    assert sorted(rows["det_score"][:2].tolist()) == [float(up)] * 2
    assert rows["counts"].tolist() == [[2, 2], [1, 1], [0, 0], [1, 0], [0, 0]]
    assert not (rows["det_score"] == float(t)).any()
    # a float64 comparison would keep float32(0.15) = 0.15000000596 > 0.15: the dict route does not, and neither do the rows
    assert float(t) > 0.15


def test_the_hundredth_row_of_a_tie_is_the_lowest_record_row(ssd):
    case = rcases.truncation_case()
    rows, want = equals_dict_route(ssd, case)
    k = case["cat_ids"].index(10)
    assert rows["counts"][k].tolist() == [100, 100, 100]
    first = np.cumsum(rows["counts"].reshape(-1)) - rows["counts"].reshape(-1)
    a = int(first[k * 3])
    tail = rows["det_score"][a + 90:a + 100]
    assert (tail == float(np.float32(0.25))).all() and rows["det_score"][a + 89] > tail[0]
    # the ten tied rows that stay are record rows 90 .. 99: their boxes, in that order
    boxes = rcases.split(case["records"])[0][0]
    scaler = np.array([480, 640, 480, 640], np.float32)
    px = boxes[90:100] * scaler
    assert np.array_equal(rows["det_box"][a + 90:a + 100, 0], px[:, 1].astype(np.int64).astype(np.float64))
    assert np.array_equal(rows["det_box"][a + 90:a + 100, 1], px[:, 0].astype(np.int64).astype(np.float64))


def test_boxes_that_a_fused_multiply_add_would_change(ssd):
    """contraction_boxes' stream; at least 4 boxes of each kind; the rows hold the UNFUSED widths and heights."""
    xmin, xmax, W, w, kind = rcases.contraction_boxes()
    assert (kind & 2).sum() >= 4 and (kind & 1).sum() >= 4, ((kind & 2).sum(), (kind & 1).sum())
    case, want = rcases.contraction_case()
    rows, _ = equals_dict_route(ssd, case)
    k = case["cat_ids"].index(20)
    first = np.cumsum(rows["counts"].reshape(-1)) - rows["counts"].reshape(-1)
    n = len(case["image_ids"])
    seen = 0
    for i, (w_i, _kind) in enumerate(want):
        a = int(first[k * n + i])
        assert rows["counts"][k, i] == len(w_i)
        assert np.array_equal(rows["det_box"][a:a + len(w_i), 2], w_i.astype(np.float64))
        assert np.array_equal(rows["det_box"][a:a + len(w_i), 3], w_i.astype(np.float64))
        assert np.array_equal(rows["det_area"][a:a + len(w_i)], (w_i * w_i).astype(np.float64))
        seen += len(w_i)
    assert seen == len(w)


def test_write_predictions_is_json_dumps_byte_for_byte(ssd):
    case = rcases.random_case(7)
    boxes, labels, scores, num = rcases.split(case["records"])
    scores[0, :3] = [1.5e-5, 3e-7, 1.0]                    # reprs with an exponent (kept at threshold 0) and without a fraction
    labels[0, :3] = [0, 1, 2]

    class Stub:
        def detect_many(self, images, score_threshold, max_batch):
            return [ssd.ssd.score_filter(b, l, s, n, score_threshold) for b, l, s, n in zip(boxes, labels, scores, num)]
    images = [np.empty((h, w, 3), np.uint8) for h, w in case["image_hw"].tolist()]
    for thr in (0.15, 0.0):
        rows = ssd.coco_eval.detection_records_many(Stub(), images, case["image_ids"], case["mapping"], thr)
        want = json.dumps(rows)[1:-1].encode()
        got = ssd.coco_rows.write_predictions(case["records"], case["image_ids"], case["image_hw"], case["mapping"], thr)
        assert isinstance(got, bytes) and got == want
        assert not any(r["image_id"] == case["image_ids"][3] for r in rows) and len(rows) > 50      # an image without detections
    assert b"e-05" in got and b"e-07" in got and b'"score": 1.0}' in got
    # no image at all, and no row at all
    assert ssd.coco_rows.write_predictions(case["records"][:0], [], case["image_hw"][:0], case["mapping"], 0.15) == b""
    assert ssd.coco_rows.write_predictions(case["records"], case["image_ids"], case["image_hw"], case["mapping"], 100.0) == b""


def bad_cases():
    """name -> (case, the image's position, the row the error names)"""
    out = {}
    for name in ("nan coordinate", "infinite score", "label past the mapping", "num_boxes -1", "num_boxes T + 1"):
        case = rcases.random_case(11)
        boxes, labels, scores, num = rcases.split(case["records"])
        T = scores.shape[1]
        i, j = 6, 2
        num[i] = max(int(num[i]), 6)
        boxes[i, :6], labels[i, :6], scores[i, :6] = np.array([0.1, 0.2, 0.5, 0.6], np.float32), 1, 0.9
        if name == "nan coordinate":
            boxes[i, j, 3] = np.nan
            boxes[i, j + 2, 0] = np.nan                     # (the lowest row is named)
        elif name == "infinite score":
            scores[i, j] = np.inf
        elif name == "label past the mapping":
            labels[i, j] = 7
        elif name == "num_boxes -1":
            num[i], j = -1, T
        else:
            num[i], j = T + 1, T
        out[name] = (case, i, j)
    return out


@pytest.mark.parametrize("name", sorted(bad_cases()))
def test_a_bad_record_raises_naming_the_image_and_the_row(ssd, name):
    case, i, j = bad_cases()[name]
    with pytest.raises(ValueError, match=r"record row %d of image %d\b" % (j, case["image_ids"][i])):
        host_rows(ssd, case)
    gt = {"images": [{"id": k, "height": h, "width": w} for k, (h, w) in zip(case["image_ids"], case["image_hw"].tolist())],
          "annotations": [], "categories": [{"id": c} for c in case["cat_ids"]]}
    with pytest.raises(ValueError, match=r"record row %d of image %d\b" % (j, case["image_ids"][i])):
        ssd.coco_metric.CocoBoxEval.from_records(gt, case["records"], case["image_ids"], case["mapping"], case["thr"])
    # garbage BEHIND num_boxes is no error: random_case itself is full of it
    host_rows(ssd, rcases.random_case(11))


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_from_records_on_the_host_gives_the_dict_routes_statistics(ssd, seed):
    gt, dets = cases.make(seed)
    sized, rec, ids, mapping, dets = rcases.from_results(gt, dets)
    metric = ssd.coco_metric
    host = metric.CocoBoxEval(gt, dets).evaluate().accumulate()
    want = host.summarize()
    ev = metric.CocoBoxEval.from_records(sized, rec, ids, mapping, 0.0)
    assert ev._dts is None
    # the packed cells are the dict route's, groundtruth included
    p, q = ev._rows_pack(ev.img_ids), ssd.coco_match.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    assert p["keys"] == q["keys"] and all(same_array(p[k], q[k]) for k in q if k != "keys")
    got = ev.evaluate().accumulate().summarize()
    assert len(got) == 12 and all(float(a) == float(b) for a, b in zip(got, want)), (got, want)
    assert list(ev.eval_imgs) == list(host.eval_imgs) and want[0] > 0
    # records in another order than the ids', a subset of the images, image sizes passed instead of read
    back = list(range(len(ids)))[::-1]
    odd = [i for i in ids if i % 2]
    part = metric.CocoBoxEval.from_records(gt, rec[back], [ids[k] for k in back], mapping, 0.0, image_hw=[(256, 256)] * len(ids))
    a, b = part.evaluate(img_ids=odd).cells(), metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd).cells()
    assert all(same_array(a[k], b[k]) for k in b)
    with pytest.raises(ValueError, match="has no 'height'"):
        metric.CocoBoxEval.from_records(gt, rec, ids, mapping, 0.0)
    with pytest.raises(ValueError, match="does not have"):
        metric.CocoBoxEval.from_records(sized, rec[:1], [10 ** 6], mapping, 0.0)
    with pytest.raises(ValueError, match="twice"):
        metric.CocoBoxEval.from_records(sized, rec[:2], [ids[0], ids[0]], mapping, 0.0)


def test_an_oversize_groundtruth_cell_takes_the_dict_route(ssd):
    gt, dets = cases.make(1)
    n = ssd.coco_match.MAX_GT + 1
    anns = gt["annotations"] + [{"image_id": 5, "category_id": 3, "bbox": [k % 50, k // 50, 20, 20], "area": 400.0, "iscrowd": 0} for k in range(n)]
    sized, rec, ids, mapping, dets = rcases.from_results(dict(gt, annotations=anns), dets)
    ev = ssd.coco_metric.CocoBoxEval.from_records(sized, rec, ids, mapping, 0.0)
    assert ev._rows is None and ev._dts
    want = ssd.coco_metric.CocoBoxEval(sized, dets).evaluate().accumulate().summarize()
    assert all(float(a) == float(b) for a, b in zip(ev.evaluate().accumulate().summarize(), want))


def test_the_entry_points_refuse_before_any_hip_call(ssd):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the calls
    never read."""
    lib, cr = ssd.lib(), ssd.coco_rows
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    names = ("records", "image_hw", "label_to_cat", "counts", "bad", "det_begin", "det_box", "det_area", "det_score")

    def call(which, n=3, T=8, num_labels=7, K=5, thr=0.15, nd=10, **kw):
        a = dict({k: fake for k in names}, **kw)
        if which == "count":
            rc = lib.ssd_coco_rows_count(a["records"], n, T, a["image_hw"], a["label_to_cat"], num_labels, K, thr, a["counts"], a["bad"], None)
        else:
            rc = lib.ssd_coco_rows_fill(a["records"], n, T, a["image_hw"], a["label_to_cat"], num_labels, K, thr, a["det_begin"], nd,
                                        a["det_box"], a["det_area"], a["det_score"], None)
        return rc, lib.ssd_last_error().decode()

    def refused(which, word, **kw):
        rc, msg = call(which, **kw)
        assert rc == -1 and msg.startswith("ssd_coco_rows_%s: " % which) and word in msg, (which, rc, msg)

    for which in ("count", "fill"):
        for name in ("records", "image_hw", "label_to_cat"):
            refused(which, name + "_dev is NULL", **{name: None})
            refused(which, name + "_dev must be 4-byte aligned", **{name: fake + 2})
        refused(which, "T must be in [1, %d]" % cr.ROWS_MAX_T, T=0)
        refused(which, "T must be in [1, %d]" % cr.ROWS_MAX_T, T=cr.ROWS_MAX_T + 1)
        refused(which, "K must be in [1, 2^20]", K=0)
        refused(which, "K must be in [1, 2^20]", K=(1 << 20) + 1)
        refused(which, "K * n_images must not pass 2^31 - 1", K=1 << 20, n=1 << 11)
        refused(which, "n_images must be in [0, 2^31 - 1]", n=-1)
        refused(which, "n_images must be in [0, 2^31 - 1]", n=1 << 31)
        refused(which, "num_labels must be in [1, 2^20]", num_labels=0)
        refused(which, "num_labels must be in [1, 2^20]", num_labels=(1 << 20) + 1)
        for thr in (np.nan, np.inf, -np.inf):
            refused(which, "score_threshold must be finite", thr=thr)
    for name in ("counts", "bad"):
        refused("count", name + "_dev is NULL", **{name: None})
        refused("count", name + "_dev must be 4-byte aligned", **{name: fake + 2})
    for name in ("det_begin", "det_box", "det_area", "det_score"):
        refused("fill", name + "_dev is NULL", **{name: None})
        refused("fill", name + "_dev must be 8-byte aligned", **{name: fake + 4})
    refused("fill", "nd must be in [0, 2^31 - 1]", nd=-1)
    refused("fill", "nd must be in [0, 2^31 - 1]", nd=1 << 31)
    # what is NOT refused returns 0 without a launch: no image (every array NULL), and a fill of no row
    none = {k: None for k in names}
    assert call("count", n=0, **none)[0] == 0 and call("fill", n=0, nd=0, **none)[0] == 0
    assert call("fill", nd=0, det_box=None, det_area=None, det_score=None)[0] == 0
