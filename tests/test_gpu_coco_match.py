"""-m gpu: ssd_coco_match (include/ssd_hip.h, "the COCO box matching") against the host loop of coco_metric.py, bit for bit: the
cells, the statistics, the IoUs, subsets, the host fallback of an oversize cell, a cell list longer than one grid pass, every
output element between guard words, streams, and coco_eval.evaluate end to end."""
import numpy as np
import pytest

from helpers import coco_match_cases as cases
from helpers import coco_match_ref as ref
from helpers import guarded

pytestmark = pytest.mark.gpu
CELL_ARRAYS = ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore")
PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15,
          "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 128}


def same_cells(a, b):
    for k in CELL_ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def sets(ssd):
    """seed -> (annotations, results, the host loop's CocoBoxEval, evaluated)"""
    out = {}
    for seed in cases.SEEDS:
        gt, dets = cases.make(seed)
        out[seed] = (gt, dets, ssd.coco_metric.CocoBoxEval(gt, dets).evaluate())
    return out


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_cells_and_statistics_equal_the_host_loop(cuda, ssd, sets, seed):
    gt, dets, host = sets[seed]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0)
    assert list(ev.eval_imgs) == list(host.eval_imgs)                  # the same keys in the same insertion order
    same_cells(ev.cells(), host.cells())
    got, want = ev.accumulate().summarize(), ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate().summarize()
    assert len(got) == 12 and all(float(g) == float(w) for g, w in zip(got, want)), (got, want)
    dev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=cuda.device("cuda", 0))
    same_cells(dev.cells(), host.cells())


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_iou_dump_is_bbox_iou_bit_for_bit(cuda, ssd, sets, seed):
    gt, dets, host = sets[seed]
    cm, metric = ssd.coco_match, ssd.coco_metric
    p = cm.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    m, i, g, dump = cm.match(p, metric.THR_L, metric.AREA_RNG, 0, want_iou=True)
    m2, i2, g2 = cm.match(p, metric.THR_L, metric.AREA_RNG, 0)
    assert np.array_equal(m, m2) and np.array_equal(i, i2) and np.array_equal(g, g2)      # the dump changes nothing else
    at = pairs = 0
    for cell in p["cells"]:
        d0, g0, D, G = int(cell["det_begin"]), int(cell["gt_begin"]), int(cell["D"]), int(cell["G"])
        want = metric.bbox_iou(p["det_box"][d0:d0 + D], p["gt_box"][g0:g0 + G], p["gt_crowd"][g0:g0 + G])
        got = dump[at:at + D * G].reshape(D, G)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64)), (d0, g0)
        at += D * G
        pairs += int(np.count_nonzero(want))
    assert at == len(dump) and pairs > 200


def test_a_subset_on_the_gpu_merges_with_the_rest(cuda, ssd, sets):
    gt, dets, host = sets[1]
    odd = [i for i in host.img_ids if i % 2]
    even = [i for i in host.img_ids if not i % 2]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd, device=0)
    same_cells(ev.cells(), ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd).cells())
    ev.merge(ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=even).cells())
    assert set(ev.eval_imgs) == set(host.eval_imgs)
    for key, want in host.eval_imgs.items():
        assert all(np.array_equal(a, b) for a, b in zip(ev.eval_imgs[key], want)), key
    assert np.array_equal(ev.accumulate().summarize(), ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate().summarize())
    none = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=[], device=0)          # no cell: nothing is launched
    assert none.eval_imgs == {} and none.cells()["keys"].shape == (0, 3)


def test_an_oversize_cell_takes_the_host_fallback_in_place(cuda, ssd, sets):
    gt, dets, _ = sets[2]
    n = ssd.coco_match.MAX_GT + 1
    img, cat = 5, 3                                             # in the middle of the cell list
    anns = [a for a in gt["annotations"] if (a["image_id"], a["category_id"]) != (img, cat)]
    anns += [{"image_id": img, "category_id": cat, "bbox": [k % 50, k // 50, 20 + k % 3, 20], "area": float((20 + k % 3) * 20), "iscrowd": int(k % 40 == 0)}
             for k in range(n)]
    dets = dets + [{"image_id": img, "category_id": cat, "bbox": [7 * k, k, 21, 20], "score": 0.3 + 0.1 * k} for k in range(5)]
    gt = dict(gt, annotations=anns)
    host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate()
    p = ssd.coco_match.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    assert p["keys"][int(np.nonzero(~p["packed"])[0][0])] == (cat, img) and np.count_nonzero(~p["packed"]) == 1
    assert 0 < p["keys"].index((cat, img)) < len(p["keys"]) - 1 and p["cells"]["G"].max() <= ssd.coco_match.MAX_GT
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0)
    assert list(ev.eval_imgs) == list(host.eval_imgs) and len(ev.eval_imgs[(cat, 0, img)][3]) == n
    same_cells(ev.cells(), host.cells())


def test_more_cells_than_one_grid_pass(cuda, ssd):
    one_pass = ssd.coco_match.GRID_CAP * ssd.coco_match.CELLS_PER_BLOCK
    gt, dets = cases.make(5, n_img=one_pass // 5, crafted=False)        # ~ 7/8 of the (image, category) pairs are cells
    host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate()
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0)
    assert len(ev.eval_imgs) // len(ssd.coco_metric.AREA_RNG) > one_pass + ssd.coco_match.CELLS_PER_BLOCK
    assert list(ev.eval_imgs) == list(host.eval_imgs)
    same_cells(ev.cells(), host.cells())


def spread(p, every=5, det_gap=3, gt_gap=2):
    """pack()'s arrays with rows of no cell in front of every `every`-th cell (and behind the last): the cells' ranges stay ascending and
    disjoint.  The gap rows hold finite boxes the kernel must never read into a result."""
    cells = p["cells"].copy()
    shift_d = np.cumsum((np.arange(len(cells)) % every == 0) * det_gap)
    shift_g = np.cumsum((np.arange(len(cells)) % every == 0) * gt_gap)
    nd, ng = len(p["det_area"]) + int(shift_d[-1]) + det_gap, len(p["gt_area"]) + int(shift_g[-1]) + gt_gap
    out = {"cells": cells, "det_box": np.full((nd, 4), 7.0), "det_area": np.full(nd, 49.0), "gt_box": np.full((ng, 4), 7.0),
           "gt_area": np.full(ng, 49.0), "gt_crowd": np.zeros(ng, np.uint8)}
    for n, cell in enumerate(p["cells"]):
        d0, g0, D, G = int(cell["det_begin"]), int(cell["gt_begin"]), int(cell["D"]), int(cell["G"])
        a, b = d0 + int(shift_d[n]), g0 + int(shift_g[n])
        cells["det_begin"][n], cells["gt_begin"][n] = a, b
        for k in ("det_box", "det_area"):
            out[k][a:a + D] = p[k][d0:d0 + D]
        for k in ("gt_box", "gt_area", "gt_crowd"):
            out[k][b:b + G] = p[k][g0:g0 + G]
    return out


@pytest.mark.parametrize("layout", ["skewed", "aligned"])
def test_every_output_is_written_between_guard_words(cuda, ssd, sets, layout):
    """Outputs prefilled with 0xFF bytes, every buffer between guard words; `skewed` puts every base at 16 (mod 32).  The numpy
    restatement leaves 0xFF in the rows of no cell and its words inside a cell never are 0xFFFF / 0xFF, so equality over the whole
    buffers says: every element of a cell written (cells with D = 0 and with G = 0 among them), every other row untouched."""
    gt, dets, host = sets[0]
    cm, metric = ssd.coco_match, ssd.coco_metric
    p = spread(cm.pack(host._gts, host._dts, host.cat_ids, host.img_ids))
    cells = p["cells"]
    assert (cells["D"] == 0).any() and (cells["G"] == 0).any() and cells["D"].max() == 100
    T, A, nd, ng = len(metric.THR_L), len(metric.AREA_RNG), len(p["det_area"]), len(p["gt_area"])
    assert nd > cells["D"].sum() and ng > cells["G"].sum()
    want_m, want_i, want_g, want_iou = ref.match(cells, p["det_box"], p["det_area"], p["gt_box"], p["gt_area"], p["gt_crowd"],
                                                 metric.THR_L, metric.AREA_RNG, want_iou=True)
    assert (want_m == 0xFFFF).sum() == A * (nd - cells["D"].sum()) and (want_g == 0xFF).sum() == A * (ng - cells["G"].sum())
    arena = guarded.Arena(cuda, cuda.device("cuda", 0), layout)
    as_bytes = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    arena.add("cells", as_bytes(cells), np.uint8, 16, "input")
    for k in ("det_box", "det_area", "gt_box", "gt_area", "gt_crowd"):
        arena.add(k, as_bytes(p[k]), np.uint8, 16, "input")
    arena.add("matched", (A * nd * 2,), np.uint8, 16, "output", fill=0xFF)
    arena.add("ignored", (A * nd * 2,), np.uint8, 16, "output", fill=0xFF)
    arena.add("gt_ignore", (A * ng,), np.uint8, 16, "output", fill=0xFF)
    arena.add("iou", (len(want_iou) * 8,), np.uint8, 16, "output", fill=0xFF)
    v = arena.view
    if layout == "skewed":
        assert all(v(k).data_ptr() % 32 == 16 for k in arena.tensors)
    cm.launch(cells, v("cells"), v("det_box"), v("det_area"), nd, v("gt_box"), v("gt_area"), v("gt_crowd"), ng, metric.THR_L, metric.AREA_RNG,
              v("matched"), v("ignored"), v("gt_ignore"), v("iou"))
    cuda.cuda.synchronize()
    arena.check()
    out = arena.outputs()
    assert np.array_equal(out["matched"].view(np.uint16).reshape(A, nd), want_m)
    assert np.array_equal(out["ignored"].view(np.uint16).reshape(A, nd), want_i)
    assert np.array_equal(out["gt_ignore"].reshape(A, ng), want_g)
    assert np.array_equal(out["iou"].view(np.uint64), want_iou.view(np.uint64))


def test_a_side_stream_and_a_second_launch_give_the_same_bits(cuda, ssd, sets):
    gt, dets, host = sets[2]
    cm, metric = ssd.coco_match, ssd.coco_metric
    p = cm.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    first = cm.match(p, metric.THR_L, metric.AREA_RNG, 0)
    second = cm.match(p, metric.THR_L, metric.AREA_RNG, 0)
    side = cuda.cuda.Stream(device=0)
    with cuda.cuda.stream(side):
        third = cm.match(p, metric.THR_L, metric.AREA_RNG, 0)
        ev = metric.CocoBoxEval(gt, dets).evaluate(device=0)
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    same_cells(ev.cells(), host.cells())


def test_coco_eval_end_to_end_with_the_gpu_metric(cuda, ssd, tmp_path):
    """coco_eval.evaluate on a tiny synthetic detector and image folder (the setup of tests/test_gpu_eval_harness.py, with the
    detector's own detections above 0.3 as the annotated objects), once with metric_device=0 and once without: identical
    statistics, byte-identical predictions files."""
    import json
    from PIL import Image
    Wt = ssd.synthetic_weights(PARAMS, seed=3, logits_bias=-4.0)
    det = ssd.Detector(Wt, config=PARAMS)
    cats = [{"id": i + 1 + (i > 10), "name": n} for i, n in enumerate(ssd.coco_eval.COCO_NAMES)]
    mapping = ssd.coco_eval.integer_to_coco_id(cats)
    rng = np.random.default_rng(23)
    images, anns, seen = [], [], 0
    for k, shape in enumerate([(128, 128, 3), (100, 151, 3), (300, 128, 3), (97, 203, 3), (128, 200, 3), (100, 151, 3)]):
        im = rng.integers(0, 256, shape, dtype=np.uint8)
        name = "%012d.png" % (k + 1)
        Image.fromarray(im).save(str(tmp_path / name))
        images.append({"id": 1000 + k, "file_name": name, "height": shape[0], "width": shape[1]})
        for r in ssd.coco_eval.detection_records(det, im, 1000 + k, mapping, score_threshold=0.3):
            x, y, w, h = r["bbox"]
            seen += 1
            if w > 0 and h > 0 and seen % 3:                    # a third of the objects stay unannotated: AP below 1
                anns.append({"id": len(anns) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"],
                             "area": float(w * h), "iscrowd": int(len(anns) % 7 == 0)})
    gt = {"images": images, "annotations": anns, "categories": cats}
    assert len(anns) > 20
    st_host = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=str(tmp_path / "pred_host.json"), max_batch=4)
    st_gpu = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=str(tmp_path / "pred_gpu.json"), max_batch=4, metric_device=0)
    assert len(st_gpu) == 12 and all(float(a) == float(b) for a, b in zip(st_gpu, st_host)), (st_gpu, st_host)
    assert st_host[0] > 0
    assert open(tmp_path / "pred_gpu.json", "rb").read() == open(tmp_path / "pred_host.json", "rb").read()
