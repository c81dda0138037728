"""-m gpu: the `timings` dictionaries of the metric family's four timed paths (voc_match.evaluate_packed, coco_match.match_device,
coco_accumulate.accumulate, coco_rows.rows_device), each on one small case: exactly the documented keys, every value but 'route' a
finite float >= 0, and the results of the timed call equal to those of the same call with timings=None, bit for bit."""
import math

import numpy as np
import pytest

from helpers import coco_match_cases as cases
from helpers import coco_rows_cases as rcases
from helpers import voc_match_cases as vcases
from helpers.voc_match_cases import feed

pytestmark = pytest.mark.gpu
CELL_ARRAYS = ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def seconds(timings, keys):
    assert set(timings) == set(keys), sorted(timings)
    for k, v in timings.items():
        if k != "route":
            assert type(v) is float and math.isfinite(v) and v >= 0, (k, v)


@pytest.fixture(scope="module")
def coco_set():
    return cases.make(0)


def test_voc_evaluate(cuda, ssd):
    images = vcases.make(0, n_img=10)                    # with the oversize cell: the host-scanned rows are uploaded too
    plain = feed(ssd.voc_match.VocEvaluator(vcases.NUM_CLASSES), images).evaluate(vcases.THR, device=0)
    timings = {}
    timed = feed(ssd.voc_match.VocEvaluator(vcases.NUM_CLASSES), images).evaluate(vcases.THR, device=0, timings=timings)
    seconds(timings, ("pack", "upload", "match", "curve", "download", "dict"))
    assert list(timed) == list(plain) and same_bits(timed["mAP"], plain["mAP"])
    for label in range(vcases.NUM_CLASSES):
        assert list(timed[label]) == list(plain[label])
        for k, v in plain[label].items():
            assert type(timed[label][k]) is type(v) and same_bits(timed[label][k], v), (label, k)


@pytest.mark.parametrize("unpack", [True, False])
def test_coco_evaluate(cuda, ssd, coco_set, unpack):
    gt, dets = coco_set
    plain, timed = ssd.coco_metric.CocoBoxEval(gt, dets), ssd.coco_metric.CocoBoxEval(gt, dets)
    plain.eval_imgs, timed.eval_imgs = {}, {}            # as evaluate() leaves it for this call
    plain._evaluate_on_gpu(plain.img_ids, 0, unpack=unpack)
    timings = {}
    timed._evaluate_on_gpu(timed.img_ids, 0, timings=timings, unpack=unpack)
    seconds(timings, ("pack", "upload", "launch", "download", "unpack") if unpack else ("pack", "upload", "launch"))
    if not unpack:
        for k in ("matched", "ignored", "gt_ignore"):
            assert timed._retained[k].is_cuda and same_bits(timed._retained[k].cpu().numpy(), plain._retained[k].cpu().numpy()), k
    a, b = timed.cells(), plain.cells()
    assert len(a["keys"]) > 0
    for k in CELL_ARRAYS:
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("route", ["retained", "upload"])
def test_coco_accumulate(cuda, ssd, coco_set, route):
    gt, dets = coco_set
    new = lambda: ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=route == "upload")
    plain = new()._accumulate_on_gpu(0)
    timings = {}
    timed = new()._accumulate_on_gpu(0, timings=timings)
    seconds(timings, ("route", "pack_order", "upload", "launch", "download"))
    assert timings["route"] == route
    assert same_bits(timed.precision, plain.precision) and same_bits(timed.recall, plain.recall)
    assert timed.precision.dtype == np.float64 and (timed.precision > 0).any()


def test_coco_rows(cuda, ssd):
    case = rcases.threshold_case()
    args = (case["records"], case["image_hw"], rcases.label_to_cat(case), len(case["cat_ids"]), case["thr"], 0)
    plain = ssd.coco_rows.rows_device(*args, image_ids=case["image_ids"])
    timings = {}
    timed = ssd.coco_rows.rows_device(*args, image_ids=case["image_ids"], timings=timings)
    seconds(timings, ("count", "scan", "fill", "download"))
    assert set(timed) == set(plain) == {"counts", "det_box", "det_area", "det_score"} and len(timed["det_score"]) > 0
    for k in ("det_box", "det_area"):
        assert timed[k].is_cuda and same_bits(timed[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for k in ("counts", "det_score"):
        assert same_bits(timed[k], plain[k]), k
