"""-m gpu: ssd_coco_rows_count / ssd_coco_rows_fill (include/ssd_hip.h, "the COCO rows") against coco_rows.rows_host, bit for bit, on
the cases of tests/test_coco_rows_host.py; more images than one grid pass; every output between guard words; streams;
CocoBoxEval.from_records on the GPU against the dict route; Detector.detect_many_records; coco_eval.evaluate(rows_device=) end to
end."""
import numpy as np
import pytest

from helpers import coco_match_cases as cases
from helpers import coco_rows_cases as rcases
from helpers import guarded

pytestmark = pytest.mark.gpu
CELL_ARRAYS = ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore")
PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15,
          "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 128}
SHAPES = [(128, 128, 3), (100, 151, 3), (300, 128, 3), (97, 203, 3), (128, 200, 3), (100, 151, 3)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def args(case):
    return case["records"], case["image_hw"], rcases.label_to_cat(case), len(case["cat_ids"]), case["thr"]


def device_rows(ssd, case, device=0):
    rows = ssd.coco_rows.rows_device(*args(case), device, image_ids=case["image_ids"])
    assert rows["det_box"].is_cuda and rows["det_area"].is_cuda and isinstance(rows["det_score"], np.ndarray)
    return dict(rows, det_box=rows["det_box"].cpu().numpy(), det_area=rows["det_area"].cpu().numpy())


def equal_rows(got, want):
    for k in ("counts", "det_box", "det_area", "det_score"):
        assert same_bits(got[k], want[k]), (k, got[k].shape, want[k].shape)


CASES = {"random 0": lambda: rcases.random_case(0), "random 1": lambda: rcases.random_case(1), "random 2": lambda: rcases.random_case(2),
         "random 3": lambda: rcases.random_case(3), "threshold": rcases.threshold_case, "truncation": rcases.truncation_case,
         "contraction": lambda: rcases.contraction_case()[0]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_device_equals_rows_host(cuda, ssd, name):
    case = CASES[name]()
    want = ssd.coco_rows.rows_host(*args(case))
    assert len(want["det_score"]) > 0
    equal_rows(device_rows(ssd, case), want)
    equal_rows(dict(device_rows(ssd, dict(case, records=cuda.from_numpy(case["records"]).cuda()))), want)      # records already on the GPU


def test_the_gpu_keeps_the_unfused_widths(cuda, ssd):
    """the contraction-sensitive boxes against the float64 emulation itself, not only against numpy's float32"""
    case, want = rcases.contraction_case()
    rows = device_rows(ssd, case)
    k, n = case["cat_ids"].index(20), len(case["image_ids"])
    first = np.cumsum(rows["counts"].reshape(-1)) - rows["counts"].reshape(-1)
    for i, (w, _kind) in enumerate(want):
        a = int(first[k * n + i])
        assert np.array_equal(rows["det_box"][a:a + len(w), 2], w.astype(np.float64)) and np.array_equal(rows["det_box"][a:a + len(w), 3], w.astype(np.float64))


@pytest.mark.parametrize("name", ["nan coordinate", "infinite score", "label past the mapping", "num_boxes -1", "num_boxes T + 1"])
def test_a_bad_record_raises_as_on_the_host(cuda, ssd, name):
    case = rcases.random_case(11)
    boxes, labels, scores, num = rcases.split(case["records"])
    T, i, j = scores.shape[1], 6, 2
    num[i] = max(int(num[i]), 6)
    boxes[i, :6], labels[i, :6], scores[i, :6] = np.array([0.1, 0.2, 0.5, 0.6], np.float32), 1, 0.9
    if name == "nan coordinate":
        boxes[i, j, 3], boxes[i, j + 2, 0] = np.nan, np.nan
    elif name == "infinite score":
        scores[i, j] = np.inf
    elif name == "label past the mapping":
        labels[i, j] = 7
    else:
        num[i], j = (-1 if name == "num_boxes -1" else T + 1), T
    for build in (ssd.coco_rows.rows_host, lambda *a, **kw: ssd.coco_rows.rows_device(*a, 0, **kw)):
        with pytest.raises(ValueError, match=r"record row %d of image %d\b" % (j, case["image_ids"][i])):
            build(*args(case), image_ids=case["image_ids"])


def many_images(n, T=4, seed=9):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 6 * T + 1), np.int32)
    boxes, labels, scores, num = rcases.split(rec)
    boxes[:, :, :2] = rng.random((n, T, 2), dtype=np.float32) * np.float32(0.5)
    boxes[:, :, 2:] = boxes[:, :, :2] + rng.random((n, T, 2), dtype=np.float32) * np.float32(0.5)
    labels[:] = rng.integers(0, 7, (n, T))
    scores[:] = rng.choice(np.array([0.1, 0.2, 0.2, 0.6], np.float32), (n, T))
    num[:] = rng.integers(0, T + 1, n)
    case = rcases._case(rec, np.stack([rng.integers(1, 700, n), rng.integers(1, 700, n)], axis=1))
    case["image_ids"] = list(range(n))
    return case


def test_more_images_than_one_grid_pass(cuda, ssd):
    cr = ssd.coco_rows
    case = many_images(cr.GRID_CAP * cr.CELLS_PER_BLOCK + 3)
    want = cr.rows_host(*args(case))
    assert (want["counts"][:, -3:] > 0).any() and (want["counts"][:, :4] > 0).any() and want["counts"].max() > 1
    equal_rows(device_rows(ssd, case), want)


@pytest.mark.parametrize("layout", ["aligned", "skewed", "skewed8"])
def test_every_output_is_written_between_guard_words(cuda, ssd, layout):
    """counts, bad and the three row arrays between guard words, prefilled with 0xFF bytes; `skewed` puts every base at 16 (mod 32),
    `skewed8` puts det_box at 8 (mod 16), where its rows go as 8-byte stores.  nd is padded by 5 rows: the rows of no cell stay 0xFF."""
    cr = ssd.coco_rows
    case = rcases.truncation_case()
    want = cr.rows_host(*args(case))
    rec, hw, l2c, K, thr = args(case)
    n, nd, pad = len(rec), len(want["det_score"]), 5
    as_bytes = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    dev = cuda.device("cuda", 0)

    def inputs(arena):
        arena.add("records", as_bytes(rec), np.uint8, 16, "input")
        arena.add("image_hw", as_bytes(hw), np.uint8, 16, "input")
        arena.add("label_to_cat", as_bytes(l2c), np.uint8, 16, "input")
    count = guarded.Arena(cuda, dev, "skewed" if layout == "skewed8" else layout)
    inputs(count)
    count.add("counts", (K * n,), np.int32, 16, "output", fill=-1)
    count.add("bad", (n,), np.int32, 16, "output", fill=-2)
    v = count.view
    cr.launch_count(v("records").view(cuda.int32).view(n, -1), v("image_hw"), v("label_to_cat").view(cuda.int32), K, thr, v("counts"), v("bad"))
    cuda.cuda.synchronize()
    count.check()
    out = count.outputs()
    assert np.array_equal(out["counts"].reshape(K, n), want["counts"]) and (out["bad"] == -1).all()

    flat = want["counts"].reshape(-1).astype(np.int64)
    fill = guarded.Arena(cuda, dev, "skewed" if layout == "skewed8" else layout)
    inputs(fill)
    fill.add("det_begin", as_bytes(np.cumsum(flat) - flat), np.uint8, 16, "input")
    if layout == "skewed8":
        fill.add("pad4", (4,), np.uint8, 4, "output", fill=0xFF)                     # the next tensor of contract 4 sits at 8 (mod 16)
    fill.add("det_box", ((nd + pad) * 32,), np.uint8, 4 if layout == "skewed8" else 16, "output", fill=0xFF)
    fill.add("det_area", ((nd + pad) * 8,), np.uint8, 16, "output", fill=0xFF)
    fill.add("det_score", ((nd + pad) * 8,), np.uint8, 16, "output", fill=0xFF)
    v = fill.view
    if layout == "skewed":
        assert all(v(k).data_ptr() % 32 == 16 for k in fill.tensors)
    if layout == "skewed8":
        assert v("det_box").data_ptr() % 16 == 8
    records = v("records").view(cuda.int32).view(n, -1)
    cr.launch_fill(records, v("image_hw"), v("label_to_cat").view(cuda.int32), K, thr, v("det_begin"), nd + pad, v("det_box"), v("det_area"),
                   v("det_score"))
    cuda.cuda.synchronize()
    fill.check()
    out = fill.outputs()
    for k, width in (("det_box", 32), ("det_area", 8), ("det_score", 8)):
        assert np.array_equal(out[k][:nd * width], as_bytes(want[k])), k
        assert (out[k][nd * width:] == 0xFF).all(), k
    # no score passes: the count writes zeros, the fill (nd == 0) writes nothing at all
    zero = guarded.Arena(cuda, dev, "skewed" if layout == "skewed8" else layout)
    inputs(zero)
    zero.add("counts", (K * n,), np.int32, 16, "output", fill=-1)
    zero.add("bad", (n,), np.int32, 16, "output", fill=-2)
    zero.add("det_begin", as_bytes(np.zeros(K * n, np.int64)), np.uint8, 16, "input")
    zero.add("det_box", (64,), np.uint8, 16, "output", fill=0xFF)
    v = zero.view
    records = v("records").view(cuda.int32).view(n, -1)
    cr.launch_count(records, v("image_hw"), v("label_to_cat").view(cuda.int32), K, 100.0, v("counts"), v("bad"))
    cr.launch_fill(records, v("image_hw"), v("label_to_cat").view(cuda.int32), K, 100.0, v("det_begin"), 0, v("det_box"), v("det_box"), v("det_box"))
    cuda.cuda.synchronize()
    zero.check()
    out = zero.outputs()
    assert (out["counts"] == 0).all() and (out["bad"] == -1).all() and (out["det_box"] == 0xFF).all()


def test_a_side_stream_and_a_second_launch_give_the_same_bits(cuda, ssd):
    case = rcases.random_case(2)
    want = ssd.coco_rows.rows_host(*args(case))
    first = device_rows(ssd, case)
    equal_rows(device_rows(ssd, case), first)
    side = cuda.cuda.Stream(device=0)
    with cuda.cuda.stream(side):
        third = device_rows(ssd, case)
    side.synchronize()
    equal_rows(third, first)
    equal_rows(third, want)


@pytest.fixture(scope="module")
def sets(ssd):
    """seed -> (annotations with sizes, records, image ids, mapping, results, the dict route evaluated and accumulated on the host)"""
    out = {}
    for seed in cases.SEEDS:
        gt, dets = cases.make(seed)
        sized, rec, ids, mapping, dets = rcases.from_results(gt, dets)
        host = ssd.coco_metric.CocoBoxEval(sized, dets).evaluate().accumulate()
        host.summarize()
        out[seed] = (sized, rec, ids, mapping, dets, host)
    return out


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_from_records_on_the_gpu_equals_the_dict_route(cuda, ssd, sets, seed):
    gt, rec, ids, mapping, dets, host = sets[seed]
    metric = ssd.coco_metric
    ev = metric.CocoBoxEval.from_records(gt, cuda.from_numpy(rec).cuda(), ids, mapping, 0.0, device=0)
    assert ev._dts is None and ev._rows["det_box"].is_cuda
    ev.evaluate(device=0, unpack=False).accumulate(device=0)
    assert "eval_imgs" not in ev.__dict__ and ev._dts is None                   # no tuple per detection on the way to the statistics
    assert same_bits(ev.precision, host.precision) and same_bits(ev.recall, host.recall)
    assert all(float(a) == float(b) for a, b in zip(ev.summarize(), host.stats)) and host.stats[0] > 0
    a, b = ev.cells(), metric.CocoBoxEval(gt, dets).evaluate(device=0, unpack=False).cells()
    for k in CELL_ARRAYS:
        assert same_bits(a[k], b[k]), k
    # a numpy block is uploaded; the host's evaluate() of a GPU-built evaluator downloads the rows
    up = metric.CocoBoxEval.from_records(gt, rec, ids, mapping, 0.0, device=cuda.device("cuda", 0))
    assert same_bits(up.evaluate().accumulate().precision, host.precision)


def test_a_subset_of_the_records_merges_with_the_rest(cuda, ssd, sets):
    gt, rec, ids, mapping, dets, host = sets[1]
    metric = ssd.coco_metric
    odd = [i for i in ids if i % 2]
    even = [i for i in ids if not i % 2]
    ev = metric.CocoBoxEval.from_records(gt, rec, ids, mapping, 0.0, device=0).evaluate(img_ids=odd, device=0, unpack=False)
    assert not ev._retained["whole"]
    mine = [k for k, i in enumerate(ids) if not i % 2]
    rest = metric.CocoBoxEval.from_records(gt, rec[mine], even, mapping, 0.0, device=0).evaluate(img_ids=even, device=0, unpack=False)
    ev.merge(rest.cells())
    assert list(sorted(ev.eval_imgs)) == list(sorted(host.eval_imgs))
    ev.accumulate(device=0)
    assert same_bits(ev.precision, host.precision) and same_bits(ev.recall, host.recall)
    # only some images evaluated at all (img_ids of the constructor): the records of the others are left out
    part = metric.CocoBoxEval.from_records(gt, rec, ids, mapping, 0.0, device=0, img_ids=odd).evaluate(device=0, unpack=False).accumulate(device=0)
    want = metric.CocoBoxEval(gt, dets, img_ids=odd).evaluate().accumulate()
    assert same_bits(part.precision, want.precision) and same_bits(part.recall, want.recall)


def test_an_oversize_groundtruth_cell_takes_the_whole_dict_route(cuda, ssd, sets):
    gt, rec, ids, mapping, dets, _ = sets[2]
    n = ssd.coco_match.MAX_GT + 1
    anns = gt["annotations"] + [{"image_id": 5, "category_id": 3, "bbox": [k % 50, k // 50, 20 + k % 3, 20], "area": float((20 + k % 3) * 20),
                                 "iscrowd": int(k % 40 == 0)} for k in range(n)]
    gt = dict(gt, annotations=anns)
    ev = ssd.coco_metric.CocoBoxEval.from_records(gt, cuda.from_numpy(rec).cuda(), ids, mapping, 0.0, device=0)
    assert ev._rows is None and ev._dts
    host = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate()
    ev.evaluate(device=0, unpack=False).accumulate(device=0)
    assert same_bits(ev.precision, host.precision) and same_bits(ev.recall, host.recall)
    assert all(float(a) == float(b) for a, b in zip(ev.summarize(), host.summarize()))


@pytest.fixture(scope="module")
def tiny(ssd):
    """the tiny detector and the six small images of test_coco_eval_end_to_end_with_the_gpu_metric"""
    det = ssd.Detector(ssd.synthetic_weights(PARAMS, seed=3, logits_bias=-4.0), config=PARAMS)
    rng = np.random.default_rng(23)
    yield det, [rng.integers(0, 256, shape, dtype=np.uint8) for shape in SHAPES]
    det.close()


def test_detect_many_records_is_pack_records_of_detect_batch(cuda, ssd, tiny):
    det, images = tiny
    rec = det.engine.new_records(len(images), "cuda:0")
    rec.fill_(-1)
    assert det.detect_many_records(images, rec, max_batch=4) is rec
    got = rec.cpu().numpy()
    filtered = det.detect_many(images, score_threshold=0.3, max_batch=4)
    for i, im in enumerate(images):
        want = ssd.ssd.pack_records(*det.detect_batch(im[None]))
        assert want.dtype == got.dtype and np.array_equal(got[i], want[0]), i
        b, l, s, n = ssd.ssd.split_records(got[i:i + 1])
        for x, y in zip(ssd.ssd.score_filter(b[0], l[0], s[0], n[0], 0.3), filtered[i]):
            assert np.array_equal(x, y)
    assert ssd.ssd.split_records(got)[3].sum() > 0
    with pytest.raises(ValueError, match="records must"):
        det.detect_many_records(images, rec[:-1], max_batch=4)
    with pytest.raises(ValueError, match="records must"):
        det.detect_many_records(images, rec.cpu(), max_batch=4)
    det.engine.set_precision("f16x3")
    try:
        with pytest.raises(ValueError, match="f32 only"):
            det.detect_many_records(images, rec)
    finally:
        det.engine.set_precision("f32")


def test_coco_eval_end_to_end_from_records(cuda, ssd, tiny, tmp_path, monkeypatch):
    """coco_eval.evaluate on the tiny detector's image folder with rows_device=0 and without: the same twelve statistics and the same
    predictions file, and the records route builds no result dict."""
    from PIL import Image
    det, frames = tiny
    cats = [{"id": i + 1 + (i > 10), "name": n} for i, n in enumerate(ssd.coco_eval.COCO_NAMES)]
    mapping = ssd.coco_eval.integer_to_coco_id(cats)
    images, anns, seen = [], [], 0
    for k, im in enumerate(frames):
        name = "%012d.png" % (k + 1)
        Image.fromarray(im).save(str(tmp_path / name))
        images.append({"id": 1000 + k, "file_name": name, "height": im.shape[0], "width": im.shape[1]})
        for r in ssd.coco_eval.detection_records(det, im, 1000 + k, mapping, score_threshold=0.3):
            x, y, w, h = r["bbox"]
            seen += 1
            if w > 0 and h > 0 and seen % 3:
                anns.append({"id": len(anns) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"],
                             "area": float(w * h), "iscrowd": int(len(anns) % 7 == 0)})
    gt = {"images": images, "annotations": anns, "categories": cats}
    assert len(anns) > 20
    a, b = str(tmp_path / "dicts.json"), str(tmp_path / "records.json")
    st_dict = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=a, max_batch=4, chunk=4, metric_device=0)
    calls = []
    monkeypatch.setattr(ssd.coco_eval, "detection_records", lambda *args, **kw: calls.append(1))
    monkeypatch.setattr(ssd.coco_eval, "result_rows", lambda *args, **kw: calls.append(1))     # (what builds the dicts, for either caller)
    st_rec = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=b, max_batch=4, chunk=4, rows_device=0)
    assert not calls
    assert len(st_rec) == 12 and all(float(x) == float(y) for x, y in zip(st_rec, st_dict)), (st_rec, st_dict)
    assert st_dict[0] > 0
    assert open(a, "rb").read() == open(b, "rb").read() and len(open(a, "rb").read()) > 1000
    st_same = ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=None, max_batch=4, rows_device=cuda.device("cuda", 0), metric_device=0)
    assert all(float(x) == float(y) for x, y in zip(st_same, st_dict))
    with pytest.raises(ValueError, match="metric_device must be None or rows_device"):
        ssd.coco_eval.evaluate(det, gt, str(tmp_path), predictions_json=None, rows_device=0, metric_device=1)
