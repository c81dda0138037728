"""The VOC-style metric without a GPU (include/ssd_hip.h, "the VOC-style metric"): the two kernels' per-lane algorithms restated in
numpy (tests/helpers/voc_match_ref.py) equal coco_eval.Evaluator.evaluate() through the real packing; the packing; VocEvaluator's
host path and its refusals; the two entry points' refusals, which come before any HIP call."""
import os
import re

import numpy as np
import pytest

from helpers import voc_match_cases as cases
from helpers import voc_match_ref as ref
from helpers.voc_match_cases import feed, rows_per_label, same_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sets(ssd):
    """seed -> (images, Evaluator.evaluate()'s dict)"""
    out = {}
    for seed in cases.SEEDS:
        images = cases.make(seed)
        out[seed] = (images, feed(ssd.coco_eval.Evaluator(cases.NUM_CLASSES), images).evaluate(cases.THR))
    return out


def test_python_constants_are_the_headers(ssd):
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    vm = ssd.voc_match
    assert (vm.MAX_GT, vm.CELLS_PER_BLOCK, vm.GRID_CAP) == tuple(value("SSD_VOC_" + n) for n in ("MAX_GT", "CELLS_PER_BLOCK", "GRID_CAP"))
    assert vm.MAX_GT == 64 * 64
    assert (vm.CELLS_PER_BLOCK, vm.GRID_CAP) == (value("SSD_COCO_CELLS_PER_BLOCK"), value("SSD_COCO_GRID_CAP"))
    assert [n for n in vm.RESULT_DTYPE.names] == re.search(r"double (ap[^;]*);\s*int64_t ([^;]*);", hdr).expand(r"\1, \2").replace(" ", "").split(",")


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_lane_algorithms_restated_equal_the_evaluator(ssd, sets, seed, monkeypatch):
    images, want = sets[seed]
    cnt = cases.counts(images, cases.NUM_CLASSES, cases.THR, ssd.coco_eval._iou_matrix, ssd.voc_match.MAX_GT)
    for name in cases.COUNTERS:
        assert cnt[name] > 0, (name, dict(cnt))
    assert 100 < len(images) < 400
    monkeypatch.setattr(ssd.voc_match, "evaluate_packed", ref.evaluate_packed)
    got = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR, device=0)
    worst = same_metrics(got, want, rows_per_label(images, cases.NUM_CLASSES))
    print("seed %d: worst |AP - host AP| / bound = %.4f" % (seed, worst))
    assert any(want[l]["AP"] > 0 for l in range(cases.NUM_CLASSES)) and want[3]["total_FP"] == 0 and want[4]["total_FN"] == 1


@pytest.mark.parametrize("thr", [0.3, 0.75, 2.0 / 3.0])
def test_other_thresholds(ssd, sets, thr, monkeypatch):
    images, _ = sets[1]
    want = feed(ssd.coco_eval.Evaluator(cases.NUM_CLASSES), images).evaluate(thr)
    monkeypatch.setattr(ssd.voc_match, "evaluate_packed", ref.evaluate_packed)
    got = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images).evaluate(thr, device=0)
    same_metrics(got, want, rows_per_label(images, cases.NUM_CLASSES))


def test_runs_without_detections_or_without_images(ssd, monkeypatch):
    monkeypatch.setattr(ssd.voc_match, "evaluate_packed", ref.evaluate_packed)
    box = np.array([[0, 0, 8, 8.0]])
    none = (np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32))
    for images in ([(box, [1]) + none, (np.zeros((0, 4)), []) + none], []):
        want = feed(ssd.coco_eval.Evaluator(3), images).evaluate()
        got = feed(ssd.voc_match.VocEvaluator(3), images).evaluate(device=0)
        assert got == want and got[1]["total_FN"] == 1 and got["mAP"] == 0.0


def test_the_packing(ssd, sets):
    images, _ = sets[0]
    vm = ssd.voc_match
    ev = feed(vm.VocEvaluator(cases.NUM_CLASSES), images)
    flat = ev._flat()
    p = vm.pack(cases.NUM_CLASSES, *flat)
    _n, gt_box, gt_label, gt_image, det_box, det_label, det_image, det_conf = flat
    n = p["n_rows"]
    assert n == len(det_conf) and sorted(p["order"].tolist()) == list(range(n))
    # the global order: per label the stable argsort(-conf) of its detections in insertion order
    at = 0
    for label in range(cases.NUM_CLASSES):
        mine = np.nonzero(det_label == label)[0]
        want = mine[np.argsort(-det_conf[mine], kind="stable")]
        seg = p["segments"][label]
        assert (int(seg["begin"]), int(seg["count"])) == (at, len(mine)) and np.array_equal(p["order"][at:at + len(mine)], want)
        assert int(seg["num_gt"]) == max(int(np.count_nonzero(gt_label == label)), 1)
        at += len(mine)
    assert np.array_equal(p["conf"], det_conf[p["order"]])
    # the cells: every (label, image) with a detection, label-major; their rows in global order; their boxes in insertion order
    cells, pos = p["cells"], p["det_pos"]
    assert len(p["fallback"]) == 1 and cells["G"].max() <= vm.MAX_GT and (cells["G"] == 0).any() and (cells["D"] > 1).any()
    assert np.array_equal(cells["det_begin"], np.cumsum(cells["D"]) - cells["D"]) and cells["det_begin"][-1] + cells["D"][-1] == len(pos)
    rows, dbox, gbox = p["fallback"][0]
    assert len(gbox) == vm.MAX_GT + 1 and sorted(pos.tolist() + rows.tolist()) == list(range(n))
    seen, last, gt_end = set(), (-1, -1), 0
    for cell in cells:
        d0, g0, D, G = (int(cell[k]) for k in ("det_begin", "gt_begin", "D", "G"))
        src = p["order"][pos[d0:d0 + D]]
        key = (int(det_label[src[0]]), int(det_image[src[0]]))
        assert D > 0 and key > last and key not in seen and g0 >= gt_end
        assert (det_label[src] == key[0]).all() and (det_image[src] == key[1]).all() and (np.diff(pos[d0:d0 + D]) > 0).all()
        assert np.array_equal(p["det_box"][d0:d0 + D], det_box[src])
        assert np.array_equal(p["gt_box"][g0:g0 + G], gt_box[(gt_label == key[0]) & (gt_image == key[1])])
        seen.add(key)
        last, gt_end = key, g0 + G
    assert len(seen) + 1 == len(set(zip(det_label.tolist(), det_image.tolist())))
    assert pos.dtype == np.int32 and p["det_box"].dtype == np.float64 and p["gt_box"].shape == (len(gt_box), 4)
    # nothing at all
    e = vm.pack(3, 0, *[np.zeros(s) for s in ((0, 4), (0,), (0,), (0, 4), (0,), (0,), (0,))])
    assert e["n_rows"] == 0 and len(e["cells"]) == 0 and e["segments"]["num_gt"].tolist() == [1, 1, 1]


def test_scan_cell_is_the_evaluators_scan(ssd):
    """the host fallback of an oversize cell against average_precision on that cell alone"""
    big = cases.make(0, n_img=0)[-1]
    gt_boxes, gt_labels, boxes, labels, scores = big
    mine, g = labels == 0, gt_boxes[gt_labels == 0]
    order = np.argsort(-scores[mine].astype(np.float64), kind="stable")
    tp, tp_iou = ssd.voc_match.scan_cell(boxes[mine][order], g, 0.5)
    want = ssd.coco_eval.average_precision({"x": g}, [("x", b, float(s)) for b, s in zip(boxes[mine], scores[mine])], 0.5)
    assert tp.tolist() == [1, 1, 0, 0] and int(tp.sum()) == len(order) - want["total_FP"]
    assert float(np.sum(tp_iou)) / 2 == want["mean_iou_for_TP"] == 1.0


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_the_host_path_is_the_evaluators_dict(ssd, sets, seed):
    images, want = sets[seed]
    got = feed(ssd.voc_match.VocEvaluator(cases.NUM_CLASSES), images).evaluate(cases.THR)
    assert got == want and list(got) == list(want)
    one = ssd.voc_match.VocEvaluator(1)
    one.add_image(np.array([[0, 0, 8, 8.0]]), [0], np.array([[0, 0, 8, 8.0]], np.float32), [0], [0.5])
    assert "mAP" not in one.evaluate() and one.evaluate()[0]["AP"] == 1.0
    one.initialize()
    assert one.images == [] and one.evaluate()[0]["total_FN"] == 1


def test_bad_rows_are_refused_by_name(ssd):
    vm = ssd.voc_match
    box = np.array([[0, 0, 8, 8.0], [4, 4, 12, 12.0]])

    def evaluator():
        ev = vm.VocEvaluator(3)
        ev.add_image(box, [0, 1], box, [0, 1], [0.5, 0.25])
        return ev
    for what, args in (("groundtruth box 1 of image 1", (np.array([[0, 0, 8, 8.0], [0, np.inf, 1, 1]]), [0, 0], box, [0, 1], [0.5, 0.5])),
                       ("box of detection 0 of image 1", (box, [0, 0], np.array([[np.nan, 0, 1, 1], [0, 0, 1, 1.0]]), [0, 1], [0.5, 0.5])),
                       ("score of detection 1 of image 1", (box, [0, 0], box, [0, 1], [0.5, np.nan]))):
        ev = evaluator()
        ev.add_image(*args)
        with pytest.raises(ValueError) as e:
            ev.evaluate(device=0)                                       # raised by the packing, before the device is looked at
        assert what + " is not finite" in str(e.value)
    for thr in (np.nan, np.inf):
        with pytest.raises(ValueError) as e:
            evaluator().evaluate(thr, device=0)
        assert "iou_threshold" in str(e.value)
    for args in ((box, [0, 3], box, [0, 1], [0.5, 0.5]), (box, [0, 1], box, [-1, 1], [0.5, 0.5])):
        with pytest.raises(KeyError):
            evaluator().add_image(*args)
        with pytest.raises(KeyError):
            ssd.coco_eval.Evaluator(3).add_image(*args)                 # the dict lookup VocEvaluator's refusal stands for
    with pytest.raises(ValueError):
        evaluator().add_image(box, [0], box, [0, 1], [0.5, 0.5])
    with pytest.raises(ValueError) as e:
        evaluator().evaluate(device="cpu")
    assert "device must be a GPU" in str(e.value)


def test_the_entry_points_refuse_before_any_hip_call(ssd):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the calls
    never read."""
    lib, vm = ssd.lib(), ssd.voc_match
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    nd, ng, n_rows = 6, 5, 8
    good = np.zeros(2, vm.CELL_DTYPE)
    good["D"], good["G"], good["det_begin"], good["gt_begin"] = [3, 3], [2, 3], [0, 3], [0, 2]

    def match(cells=good, **kw):
        a = dict(cells_host=cells.ctypes.data, cells_dev=fake, det_box=fake, det_pos=fake, nd=nd, gt_box=fake, ng=ng, thr=0.5, tp=fake,
                 tp_iou=fake, n_rows=n_rows, n_cells=len(cells))
        a.update(kw)
        rc = lib.ssd_voc_match(a["cells_host"], a["cells_dev"], a["n_cells"], a["det_box"], a["det_pos"], a["nd"], a["gt_box"], a["ng"], a["thr"],
                               a["tp"], a["tp_iou"], a["n_rows"], None)
        return rc, lib.ssd_last_error().decode()

    def refused(call, fn, word, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(fn + ": ") and word in msg, (rc, msg)

    m = lambda word, **kw: refused(match, "ssd_voc_match", word, **kw)
    for name, arg in (("cells_host", "cells_host"), ("cells_dev", "cells_dev"), ("det_box", "det_box_dev"), ("det_pos", "det_pos_dev"),
                      ("gt_box", "gt_box_dev"), ("tp", "tp_dev"), ("tp_iou", "tp_iou_dev")):
        m(arg + " is NULL", **{name: None})
    m("det_pos_dev must be 4-byte aligned", det_pos=fake + 2)
    m("tp_iou_dev must be 8-byte aligned", tp_iou=fake + 4)
    m("gt_box_dev must be 8-byte aligned", gt_box=fake + 4)
    m("cells_dev must be 8-byte aligned", cells_dev=fake + 4)
    m("n_cells must be in [0, 2^40]", n_cells=-1)
    m("nd must be in [0, 2^40]", nd=-1)
    m("ng must be in [0, 2^40]", ng=2 ** 40 + 1)
    m("n_rows must be in [0, 2^31 - 1]", n_rows=2 ** 31)
    m("nd must be at most n_rows", n_rows=5)
    for thr in (float("nan"), float("inf"), -float("inf")):
        m("thr must be finite", thr=thr)

    def cells(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k] = v
        return c
    m("cell 0: D must not be negative", cells=cells(D=[-1, 3]))
    m("cell 1: G must be in [0, %d]" % vm.MAX_GT, cells=cells(G=[2, vm.MAX_GT + 1]))
    m("cell 1: G must be in [0, %d]" % vm.MAX_GT, cells=cells(G=[2, -1]))
    m("cell 1: det_begin must be the end of the cell before", cells=cells(det_begin=[0, 2]))
    m("cell 1: det_begin must be the end of the cell before", cells=cells(det_begin=[0, 4]))
    m("cell 0: det_begin must be the end of the cell before", cells=cells(det_begin=[1, 3]))
    m("cell 1: det_begin + D runs past nd", cells=cells(D=[3, 4]))
    m("the cells' detection ranges end at 5, not at nd", cells=cells(D=[3, 2]))
    m("cell 1: gt_begin overlaps", cells=cells(gt_begin=[0, 1]))
    m("cell 1: gt_begin + G runs past ng", cells=cells(gt_begin=[0, 3]))
    assert match(n_cells=0, nd=0, cells_host=None, cells_dev=None)[0] == 0          # nothing to do: nothing enqueued

    segs = np.zeros(3, vm.SEGMENT_DTYPE)
    segs["begin"], segs["count"], segs["num_gt"] = [0, 3, 3], [3, 0, 5], [1, 1, 7]

    def curve(segments=segs, **kw):
        a = dict(segments_host=segments.ctypes.data, segments_dev=fake, n_labels=len(segments), tp=fake, tp_iou=fake, conf=fake, n_rows=n_rows,
                 results=fake)
        a.update(kw)
        rc = lib.ssd_voc_curve(a["segments_host"], a["segments_dev"], a["n_labels"], a["tp"], a["tp_iou"], a["conf"], a["n_rows"], a["results"], None)
        return rc, lib.ssd_last_error().decode()

    c = lambda word, **kw: refused(curve, "ssd_voc_curve", word, **kw)
    for name, arg in (("segments_host", "segments_host"), ("segments_dev", "segments_dev"), ("tp", "tp_dev"), ("tp_iou", "tp_iou_dev"),
                      ("conf", "conf_dev"), ("results", "results_dev")):
        c(arg + " is NULL", **{name: None})
    c("conf_dev must be 8-byte aligned", conf=fake + 4)
    c("results_dev must be 8-byte aligned", results=fake + 4)
    c("n_labels must be in [0, 2^24]", n_labels=-1)
    c("n_labels must be in [0, 2^24]", n_labels=2 ** 24 + 1)
    c("n_rows must be in [0, 2^31 - 1]", n_rows=-1)

    def segments(**kw):
        s = segs.copy()
        for k, v in kw.items():
            s[k] = v
        return s
    c("segment 1: count must not be negative", segments=segments(count=[3, -1, 5]))
    c("segment 0: begin must not be negative", segments=segments(begin=[-1, 3, 3]))
    c("segment 2: begin + count runs past n_rows", segments=segments(count=[3, 0, 6]))
    c("segment 2: num_gt must be in [1, 2^40]", segments=segments(num_gt=[1, 1, 0]))
    assert curve(n_labels=0, segments_host=None, segments_dev=None, results=None)[0] == 0


def test_the_wiring_defaults_to_off(ssd):
    import inspect
    import ssd_amd.evaluation
    import ssd_amd.train
    assert inspect.signature(ssd_amd.evaluation.evaluate).parameters["metric_device"].default is None
    assert inspect.signature(ssd.Trainer.__init__).parameters["metric_device"].default is None
    assert inspect.signature(ssd.voc_match.VocEvaluator.evaluate).parameters["device"].default is None
    for module in (ssd_amd.evaluation, ssd_amd.train):
        assert '"--gpu-metric"' in inspect.getsource(module.main) and "store_true" in inspect.getsource(module.main)
