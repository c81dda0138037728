"""-m gpu: ssd_coco_accumulate (include/ssd_hip.h, "the COCO accumulation") against CocoBoxEval.accumulate() of coco_metric.py, bit
for bit: the three random sets and the hand-built categories, both routes of accumulate(device=), a fallback cell, merged subsets,
the entry point's bounds, an item list longer than one grid pass, every output element between guard words, streams, the lazy
eval_imgs, and coco_eval.evaluate end to end."""
import numpy as np
import pytest

from helpers import coco_accumulate_cases as acases
from helpers import coco_accumulate_ref as aref
from helpers import coco_match_cases as cases
from helpers import guarded

pytestmark = pytest.mark.gpu
SETS = tuple(cases.SEEDS) + ("hand",)
CELL_ARRAYS = ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore")
PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15,
          "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 128}


@pytest.fixture(scope="module")
def sets(ssd):
    """name -> (annotations, results, the host's CocoBoxEval evaluated, accumulated and summarized)"""
    out = {}
    for name in SETS:
        gt, dets = acases.hand_built() if name == "hand" else cases.make(name)
        host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate()
        host.summarize()
        out[name] = (gt, dets, host)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_result(ev, host):
    assert same_bits(ev.precision, host.precision), np.argwhere(ev.precision.view(np.uint64) != host.precision.view(np.uint64))[:5]
    assert same_bits(ev.recall, host.recall), np.argwhere(ev.recall.view(np.uint64) != host.recall.view(np.uint64))[:5]
    assert np.array_equal(ev.precision, host.precision) and np.array_equal(ev.recall, host.recall)


def route(ev, device=0):
    timings = {}
    ev._accumulate_on_gpu(device, timings=timings)
    return timings["route"]


@pytest.mark.parametrize("name", SETS)
def test_precision_recall_and_statistics_equal_the_host(cuda, ssd, sets, name):
    gt, dets, host = sets[name]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False).accumulate(device=0)
    same_result(ev, host)
    got = ev.summarize()
    assert len(got) == 12 and all(float(g) == float(w) for g, w in zip(got, host.stats)), (got, host.stats)
    assert "eval_imgs" not in ev.__dict__                                # the twelve statistics without the tuples
    dev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=cuda.device("cuda", 0), unpack=False).accumulate(device=cuda.device("cuda", 0))
    same_result(dev, host)


@pytest.mark.parametrize("name", SETS)
def test_the_retained_route_and_the_upload_route_agree(cuda, ssd, sets, name):
    gt, dets, host = sets[name]
    kept = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False)
    assert route(kept) == "retained"
    same_result(kept, host)
    unpacked = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0)          # unpack=True keeps nothing on the GPU
    assert route(unpacked) == "upload"
    same_result(unpacked, host)
    from_host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate()                 # host evaluate() + accumulate(device=0)
    assert route(from_host) == "upload"
    same_result(from_host, host)
    assert all(float(g) == float(w) for g, w in zip(from_host.summarize(), host.stats))


def test_a_fallback_cell_takes_the_upload_route(cuda, ssd, sets):
    gt, dets, _ = sets[2]
    n = ssd.coco_match.MAX_GT + 1                                                # 257 groundtruth boxes in one cell
    img, cat = 5, 3
    anns = [a for a in gt["annotations"] if (a["image_id"], a["category_id"]) != (img, cat)]
    anns += [{"image_id": img, "category_id": cat, "bbox": [k % 50, k // 50, 20 + k % 3, 20], "area": float((20 + k % 3) * 20), "iscrowd": int(k % 40 == 0)}
             for k in range(n)]
    dets = dets + [{"image_id": img, "category_id": cat, "bbox": [7 * k, k, 21, 20], "score": 0.3 + 0.1 * k} for k in range(5)]
    gt = dict(gt, annotations=anns)
    host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate()
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False)
    assert not ev._retained["whole"] and route(ev) == "upload"
    same_result(ev, host)
    assert len(ev.eval_imgs[(cat, 0, img)][3]) == n


def test_a_subset_on_the_gpu_merged_with_host_cells(cuda, ssd, sets):
    gt, dets, host = sets[1]
    odd = [i for i in host.img_ids if i % 2]
    even = [i for i in host.img_ids if not i % 2]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd, device=0, unpack=False)
    assert not ev._retained["whole"]
    ev.merge(ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=even).cells())
    assert ev._retained is None and set(ev.eval_imgs) == set(host.eval_imgs) and route(ev) == "upload"
    same_result(ev, host)
    # a subset alone: accumulate() runs over all img_ids, the cells of the others are simply absent -- on both paths
    part = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd, device=0, unpack=False).accumulate(device=0)
    same_result(part, ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(img_ids=odd).accumulate())


def test_lazy_cells_equal_the_unpacked_ones(cuda, ssd, sets):
    gt, dets, host = sets[0]
    lazy = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False)
    assert "eval_imgs" not in lazy.__dict__
    a, b = lazy.cells(), ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=True).cells()
    assert isinstance(lazy.__dict__["eval_imgs"], dict) and list(lazy.eval_imgs) == list(host.eval_imgs)
    for k in CELL_ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert route(lazy) == "retained"                                      # building the tuples gives nothing up
    same_result(lazy, host)
    lazy.eval_imgs = dict(host.eval_imgs)                                 # a caller's own dict: what the GPU holds is not it any more
    assert route(lazy) == "upload" and lazy._retained is None
    same_result(lazy, host)
    same_result(ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False).accumulate(), host)      # host accumulate() builds them


def flat_case(ssd, seed, det_counts, gt_counts, T, A, max_dets, rec_thr):
    ca = ssd.coco_accumulate
    f = acases.flat(seed, det_counts, gt_counts, T, A, ca.SEGMENT_DTYPE)
    want = aref.accumulate(f["segments"], f["order"], f["rank"], f["matched"], f["ignored"], f["gt_ignore"], T, max_dets, rec_thr)
    got = ca.accumulate(f, f["matched"], f["ignored"], f["gt_ignore"], T, A, max_dets, rec_thr, 0)
    return f, got, want


def test_more_items_than_one_grid_pass(cuda, ssd):
    ca = ssd.coco_accumulate
    rng = np.random.default_rng(3)
    K, T, A, max_dets = 400, 2, 4, (1, 10, 100)
    assert K * A * len(max_dets) > ca.GRID_CAP * ca.CELLS_PER_BLOCK + ca.CELLS_PER_BLOCK
    f, got, want = flat_case(ssd, 11, rng.integers(0, 6, K), rng.integers(0, 4, K), T, A, max_dets, ssd.coco_metric.REC_THRS)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert (want[1] == -1).any() and (want[1] > 0).any() and (f["segments"]["det_count"] == 0).any()


def test_the_bounds_of_every_setting(cuda, ssd):
    """T = 16, M = 4, R = 128 with thresholds below 0 (c_r = 0) and above 1 (no position), A = 1; segments of 0, 1, 63, 64, 65 and
    300 rows; and the smallest call: T = A = M = R = 1."""
    rec = np.linspace(-0.1, 1.1, 128)
    f, got, want = flat_case(ssd, 5, [0, 1, 63, 64, 65, 300, 0], [4, 1, 7, 0, 100, 150, 0], 16, 1, (1, 2, 50, 100), rec)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert got[0].shape == (16, 128, 7, 1, 4) and (want[0][:, 0] > 0).any() and (want[0][:, -1] == 0).any()
    f, got, want = flat_case(ssd, 6, [70, 5], [3, 2], 1, 1, (100,), [0.5])
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[0].shape == (1, 1, 2, 1, 1)
    # K = 0: nothing is launched, the outputs are empty
    f, got, want = flat_case(ssd, 7, [], [], 3, 2, (1, 10), rec)
    assert got[0].shape == (3, 128, 0, 2, 2) and got[1].shape == (3, 0, 2, 2)


@pytest.mark.parametrize("layout", ["skewed", "aligned"])
def test_every_output_is_written_between_guard_words(cuda, ssd, sets, layout):
    """Outputs prefilled with 0xFF bytes (a NaN no result is), every buffer between guard words; `skewed` puts every base at 16
    (mod 32).  Equality with the host's arrays over the whole buffers says every element was written; check() says nothing else was."""
    gt, dets, host = sets["hand"]
    ca, metric = ssd.coco_accumulate, ssd.coco_metric
    T, A, M, R, K = len(metric.IOU_THRS), len(metric.AREA_RNG), len(metric.MAX_DETS), len(metric.REC_THRS), len(host.cat_ids)
    q = ca.pack_cells(host.cells(), host.cat_ids, host.img_ids, A)
    arena = guarded.Arena(cuda, cuda.device("cuda", 0), layout)
    as_bytes = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    for k in ("segments", "order", "rank", "matched", "ignored", "gt_ignore"):
        arena.add(k, as_bytes(q[k]), np.uint8, 16, "input")
    arena.add("rec_thr", as_bytes(np.asarray(metric.REC_THRS, np.float64)), np.uint8, 16, "input")
    arena.add("precision", (T * R * K * A * M * 8,), np.uint8, 16, "output", fill=0xFF)
    arena.add("recall", (T * K * A * M * 8,), np.uint8, 16, "output", fill=0xFF)
    v = arena.view
    if layout == "skewed":
        assert all(v(k).data_ptr() % 32 == 16 for k in arena.tensors)
    ca.launch(q["segments"], v("segments"), v("order"), v("rank"), v("matched"), v("ignored"), q["nd"], v("gt_ignore"), q["ng"], T, A,
              metric.MAX_DETS, metric.REC_THRS, v("rec_thr"), v("precision"), v("recall"))
    cuda.cuda.synchronize()
    arena.check()
    out = arena.outputs()
    assert np.array_equal(out["precision"].view(np.uint64), host.precision.reshape(-1).view(np.uint64))
    assert np.array_equal(out["recall"].view(np.uint64), host.recall.reshape(-1).view(np.uint64))


def test_a_side_stream_and_a_second_launch_give_the_same_bits(cuda, ssd, sets):
    gt, dets, host = sets[2]
    metric = ssd.coco_metric
    ev = metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False)
    first = ev.accumulate(device=0)
    p1, r1 = first.precision.copy(), first.recall.copy()
    ev.accumulate(device=0)
    assert same_bits(ev.precision, p1) and same_bits(ev.recall, r1)
    side = cuda.cuda.Stream(device=0)
    with cuda.cuda.stream(side):
        third = metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False).accumulate(device=0)
    side.synchronize()
    assert same_bits(third.precision, p1) and same_bits(third.recall, r1)
    same_result(third, host)


def test_coco_eval_end_to_end_with_the_gpu_metric(cuda, ssd, tmp_path, monkeypatch):
    """coco_eval.evaluate on the tiny synthetic detector and image folder of tests/test_gpu_coco_match.py, once with metric_device=0
    and once without: identical statistics; the GPU run goes through accumulate(device=) and never builds eval_imgs."""
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
            if w > 0 and h > 0 and seen % 3:
                anns.append({"id": len(anns) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"],
                             "area": float(w * h), "iscrowd": int(len(anns) % 7 == 0)})
    gt = {"images": images, "annotations": anns, "categories": cats}
    assert len(anns) > 20
    seen_ev = []
    real = ssd.coco_metric.CocoBoxEval._accumulate_on_gpu

    def spy(self, device, timings=None):
        seen_ev.append(self)
        return real(self, device, timings={} if timings is None else timings)
    monkeypatch.setattr(ssd.coco_metric.CocoBoxEval, "_accumulate_on_gpu", spy)
    st_host = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=None, max_batch=4)
    assert not seen_ev
    st_gpu = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=None, max_batch=4, metric_device=0)
    assert len(st_gpu) == 12 and all(float(a) == float(b) for a, b in zip(st_gpu, st_host)), (st_gpu, st_host)
    assert st_host[0] > 0
    assert len(seen_ev) == 1 and "eval_imgs" not in seen_ev[0].__dict__
