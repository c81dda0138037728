"""The COCO box matching without a GPU (include/ssd_hip.h, "the COCO box matching"): the kernel's per-lane algorithm restated in
numpy (tests/helpers/coco_match_ref.py) equals CocoBoxEval.evaluate() through the real packing and unpacking; the packing; the
entry point's refusals, which come before any HIP call; and the host path, unchanged."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import coco_match_cases as cases
from helpers import coco_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL_ARRAYS = ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore")


def same_cells(a, b):
    for k in CELL_ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def ref_match(unpack_bits):
    """coco_match.match with the numpy restatement in the kernel's place"""
    def match(p, thr, area_rng, device, want_iou=False, timings=None):
        m, i, g = ref.match(p["cells"], p["det_box"], p["det_area"], p["gt_box"], p["gt_area"], p["gt_crowd"], thr, area_rng)
        return unpack_bits(m, len(thr)), unpack_bits(i, len(thr)), g.astype(bool)
    return match


@pytest.fixture(scope="module")
def sets(ssd):
    """seed -> (annotations, results, the host loop's cells)"""
    out = {}
    for seed in cases.SEEDS:
        gt, dets = cases.make(seed)
        out[seed] = (gt, dets, ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().cells())
    return out


def test_python_constants_are_the_headers(ssd):
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    cm = ssd.coco_match
    assert (cm.MAX_DET, cm.MAX_GT, cm.MAX_THR, cm.MAX_AREA, cm.CELLS_PER_BLOCK, cm.GRID_CAP) == tuple(
        value("SSD_COCO_" + n) for n in ("MAX_DET", "MAX_GT", "MAX_THR", "MAX_AREA", "CELLS_PER_BLOCK", "GRID_CAP"))
    assert cm.MAX_DET == ssd.coco_metric.MAX_DETS[-1] and cm.MAX_GT >= 128
    assert len(ssd.coco_metric.THR_L) <= cm.MAX_THR and len(ssd.coco_metric.AREA_RNG) <= cm.MAX_AREA
    assert len(ssd.coco_metric.THR_L) * len(ssd.coco_metric.AREA_RNG) <= 64


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_lane_algorithm_restated_equals_the_host_loop(ssd, sets, seed, monkeypatch):
    gt, dets, want = sets[seed]
    monkeypatch.setattr(ssd.coco_match, "match", ref_match(ssd.coco_match.unpack_bits))
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0)
    same_cells(ev.cells(), want)
    host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate()
    assert list(ev.eval_imgs) == list(host.eval_imgs)                  # the same keys in the same insertion order
    assert np.array_equal(ev.accumulate().summarize(), host.accumulate().summarize())
    # ... on a set that takes every branch of the scan
    cnt = cases.branch_counts(host, ssd.coco_metric)
    for name in cases.BRANCHES:
        assert cnt[name] > 0, (name, dict(cnt))
    assert len(gt["annotations"]) < 400 and len(dets) < 600


def test_one_sort_orders_and_truncates_like_the_per_cell_argsort(ssd, sets):
    gt, dets, _ = sets[0]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets)
    p = ssd.coco_match.pack(ev._gts, ev._dts, ev.cat_ids, ev.img_ids)
    assert p["packed"].all() and len(p["cells"]) == len(p["keys"])
    tied = over = 0
    for (cat, img), cell in zip(p["keys"], p["cells"]):
        dts, gts = ev._dts.get((img, cat), []), ev._gts.get((img, cat), [])
        scores = np.array([d[2] for d in dts], np.float64)
        order = np.argsort(-scores, kind="mergesort")[:100]
        a, b = int(cell["det_begin"]), int(cell["det_begin"]) + int(cell["D"])
        assert cell["D"] == len(order) and cell["G"] == len(gts)
        assert np.array_equal(p["det_score"][a:b], scores[order])
        assert np.array_equal(p["det_box"][a:b], np.array([dts[i][0] for i in order], np.float64).reshape(-1, 4))
        assert np.array_equal(p["det_area"][a:b], np.array([dts[i][1] for i in order], np.float64))
        c = int(cell["gt_begin"])
        assert np.array_equal(p["gt_box"][c:c + len(gts)], np.array([g[0] for g in gts], np.float64).reshape(-1, 4))
        assert np.array_equal(p["gt_area"][c:c + len(gts)], np.array([g[1] for g in gts], np.float64))
        assert np.array_equal(p["gt_crowd"][c:c + len(gts)], np.array([g[2] != 0 for g in gts], np.uint8))
        tied += len(set(scores.tolist())) < len(scores)
        over += len(dts) > 100
    assert tied > 0 and over > 0
    cells = p["cells"]
    assert np.array_equal(cells["det_begin"], np.cumsum(cells["D"]) - cells["D"]) and cells["det_begin"][-1] + cells["D"][-1] == len(p["det_area"])
    assert np.array_equal(cells["gt_begin"], np.cumsum(cells["G"]) - cells["G"]) and cells["gt_begin"][-1] + cells["G"][-1] == len(p["gt_area"])
    assert p["keys"] == sorted(p["keys"])


def test_a_subset_packs_only_its_cells(ssd, sets):
    gt, dets, _ = sets[1]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets)
    odd = [i for i in ev.img_ids if i % 2]
    p = ssd.coco_match.pack(ev._gts, ev._dts, ev.cat_ids, odd)
    full = ssd.coco_match.pack(ev._gts, ev._dts, ev.cat_ids, ev.img_ids)
    assert p["keys"] == [k for k in full["keys"] if k[1] % 2] and 0 < len(p["keys"]) < len(full["keys"])
    assert len(p["det_area"]) == sum(min(len(v), 100) for (img, _c), v in ev._dts.items() if img % 2)
    assert len(p["gt_area"]) == sum(len(v) for (img, _c), v in ev._gts.items() if img % 2)


@pytest.mark.parametrize("field,what", [("bbox", "box of detection"), ("score", "score of detection"), ("gtbox", "box of groundtruth box")])
def test_a_non_finite_row_is_refused_by_name(ssd, sets, field, what):
    gt, dets, _ = sets[2]
    gt = dict(gt, annotations=[dict(a) for a in gt["annotations"]])
    dets = [dict(d) for d in dets]
    if field == "gtbox":
        row = gt["annotations"][17]
        row["bbox"] = [row["bbox"][0], float("inf"), row["bbox"][2], row["bbox"][3]]
        same = [a for a in gt["annotations"] if (a["image_id"], a["category_id"]) == (row["image_id"], row["category_id"])]
    else:
        row = dets[23]
        if field == "bbox":
            row["bbox"] = [float("nan")] + list(row["bbox"][1:])
        else:
            row["score"] = float("nan")
        same = [d for d in dets if (d["image_id"], d["category_id"]) == (row["image_id"], row["category_id"])]
    pos = [k for k, r in enumerate(same) if r is row][0]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets)
    with pytest.raises(ValueError) as e:
        ev.evaluate(device=0)
    assert "%s %d of image %r, category %r" % (what, pos, row["image_id"], row["category_id"]) in str(e.value)


def test_the_entry_point_refuses_before_any_hip_call(ssd):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the call
    never reads."""
    lib, cm = ssd.lib(), ssd.coco_match
    nd, ng = 6, 5
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    thr = np.array(ssd.coco_metric.THR_L, np.float64)
    rng = np.array(ssd.coco_metric.AREA_RNG, np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    good = np.zeros(2, cm.CELL_DTYPE)
    good["D"], good["G"], good["det_begin"], good["gt_begin"] = [3, 3], [2, 3], [0, 3], [0, 2]

    def call(cells=good, T=len(thr), A=len(rng), **kw):
        a = dict(cells_host=cells.ctypes.data, cells_dev=fake, det_box=fake, det_area=fake, gt_box=fake, gt_area=fake, gt_crowd=fake,
                 thr=thr.ctypes.data_as(dp), rng=rng.ctypes.data_as(dp), matched=fake, ignored=fake, gt_ignore=fake)
        a.update(kw)
        rc = lib.ssd_coco_match(a["cells_host"], a["cells_dev"], len(cells), a["det_box"], a["det_area"], nd, a["gt_box"], a["gt_area"],
                                a["gt_crowd"], ng, a["thr"], T, a["rng"], A, a["matched"], a["ignored"], a["gt_ignore"], None, None)
        return rc, lib.ssd_last_error().decode()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("ssd_coco_match: ") and word in msg, (rc, msg)

    for name, arg in (("cells_host", "cells_host"), ("cells_dev", "cells_dev"), ("det_box", "det_box_dev"), ("det_area", "det_area_dev"),
                      ("gt_box", "gt_box_dev"), ("gt_area", "gt_area_dev"), ("gt_crowd", "gt_crowd_dev"), ("matched", "matched_dev"),
                      ("ignored", "ignored_dev"), ("gt_ignore", "gt_ignore_dev")):
        refused(arg + " is NULL", **{name: None})
    refused("thr_host is NULL", thr=None)
    refused("area_rng_host is NULL", rng=None)
    refused("matched_dev must be 2-byte aligned", matched=fake + 1)
    refused("det_box_dev must be 8-byte aligned", det_box=fake + 4)
    wide = np.zeros(32, np.float64)               # thresholds and bounds for the calls whose T or A is past the real arrays
    wp = wide.ctypes.data_as(dp)
    refused("T must be in [1, 16]", T=0)
    refused("T must be in [1, 16]", T=17, A=1, thr=wp)
    refused("A must be in [1, 4]", A=0)
    refused("A must be in [1, 4]", A=5, rng=wp)
    refused("T * A must be at most 64", T=17, A=4, thr=wp)
    refused("T * A must be at most 64", T=13, A=5, thr=wp, rng=wp)

    def cells(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k] = v
        return c
    refused("cell 1: D must be in [0, 100]", cells=cells(D=[3, 101]))
    refused("cell 0: D must be in [0, 100]", cells=cells(D=[-1, 3]))
    refused("cell 1: G must be in [0, %d]" % cm.MAX_GT, cells=cells(G=[2, cm.MAX_GT + 1]))
    refused("cell 1: det_begin overlaps", cells=cells(det_begin=[0, 2]))
    refused("cell 1: gt_begin overlaps", cells=cells(gt_begin=[0, 1]))
    refused("cell 1: det_begin + D runs past nd", cells=cells(det_begin=[0, 4]))
    refused("cell 1: gt_begin + G runs past ng", cells=cells(gt_begin=[0, 3]))
    refused("cell 0: det_begin overlaps", cells=cells(det_begin=[-1, 3]))


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_the_host_path_is_unchanged(ssd, sets, seed):
    gt, dets, want = sets[seed]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets)
    same_cells(ev.evaluate(device=None).cells(), want)
    odd = [i for i in ev.img_ids if i % 2]
    same_cells(ev.evaluate(odd, None).cells(), ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd).cells())
