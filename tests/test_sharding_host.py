"""The sharding layer without a GPU: the round-robin chunk assignment, detect_many_sharded and coco_eval.evaluate over
gloo ranks with a stand-in detector, and CocoBoxEval's subset evaluation plus merge."""
import io
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import sharding_stub  # noqa: E402


# ----------------------------------------------------------------------------- assignment
@pytest.mark.parametrize("world", range(1, 9))
def test_chunk_assignment_covers_and_restores(ssd, world):
    for chunk in (1, 2, 3, 5, 8):
        for total in sorted({0, 1, 2, chunk - 1, chunk, 7, 23, 64, world * chunk * 2 + 1}):
            locals_ = [[i for i, _x in ssd.ChunkAssignment(world, r, chunk).select(range(total))] for r in range(world)]
            flat = [i for part in locals_ for i in part]
            assert sorted(flat) == list(range(total)), (world, chunk, total)          # every image exactly once
            for r, part in enumerate(locals_):
                a = ssd.ChunkAssignment(world, r, chunk)
                assert all(a.owner(i) == r == (i // chunk) % world for i in part)
                assert a.count(total) == len(part)
            counts = [len(p) for p in locals_]
            a = ssd.ChunkAssignment(world, 0, chunk)
            assert a.input_index(counts).tolist() == flat
            assert a.to_input_order(flat, counts) == list(range(total))
    a = ssd.ChunkAssignment(world, world - 1, 2)
    if world > 1:
        with pytest.raises(ValueError):
            a.input_index([0] * (world - 1) + [2])        # the last rank cannot own images while rank 0 has none
    with pytest.raises(ValueError):
        ssd.ChunkAssignment(world, world, 2)


# ----------------------------------------------------------------------------- gloo workers
def _worker(rank, world, port, q, task):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import ssd_amd
    from helpers import sharding_stub as stub
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        if task == "detect":
            det = stub.StubDetector(T=7)
            out = []
            for n_local, chunk, max_batch in _DETECT_CASES[world]:
                mine = stub.images(1000 * world + 10 * rank + chunk, n_local[rank])
                got = ssd_amd.detect_many_sharded(det, mine, score_threshold=0.3, max_batch=max_batch, chunk=chunk)
                out.append(got)
            q.put((rank, pickle.dumps(out)))
        else:
            gt, store = _coco_case()
            det = stub.StubDetector(T=7)
            path = os.path.join(task, "pred_w%d.json" % world)
            stats = ssd_amd.coco_eval.evaluate(det, gt, "", read_image=store.__getitem__, predictions_json=path, max_batch=4,
                                               read_workers=2, group=dist.group.WORLD, chunk=3)
            q.put((rank, pickle.dumps(stats)))
    finally:
        dist.destroy_process_group()


# per world: (images per rank, chunk, max_batch); uneven, with empty ranks and ragged last rounds
_DETECT_CASES = {2: [((11, 4), 3, 2), ((0, 5), 4, 8), ((0, 0), 2, 2), ((9, 9), 64, 4)],
                 3: [((7, 0, 5), 2, 2), ((1, 13, 2), 5, 4)]}


def _spawn(world, task):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 20000 + (os.getpid() * 7 + world * 131 + len(task)) % 20000
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, task)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(60)
    assert all(p.exitcode == 0 for p in procs)
    return [pickle.loads(res[r]) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_detect_many_sharded_gloo_equals_concatenation(world):
    per_rank = _spawn(world, "detect")
    det = sharding_stub.StubDetector(T=7)
    lengths = set()
    for c, (n_local, chunk, _mb) in enumerate(_DETECT_CASES[world]):
        every = [im for r in range(world) for im in sharding_stub.images(1000 * world + 10 * r + chunk, n_local[r])]
        want = det.detect_many(every, score_threshold=0.3)
        lengths |= {len(w[2]) for w in want}
        for r in range(world):
            got = per_rank[r][c]
            assert len(got) == len(want)
            for g, w in zip(got, want):
                for u, v in zip(g, w):
                    assert u.dtype == v.dtype and np.array_equal(u, v)
    assert 0 in lengths and len(lengths) > 3             # varying lengths, zero detections included


def _coco_case():
    """A synthetic COCO split whose groundtruth follows the stand-in detector's boxes (jittered, some crowd) so that AP is
    not trivially 0; the images come from an in-memory store keyed by file name."""
    from ssd_amd import coco_eval
    det = sharding_stub.StubDetector(T=7)
    imgs = sharding_stub.images(77, 17)
    cats = [{"id": 3 * k + 1, "name": n} for k, n in enumerate(coco_eval.COCO_NAMES)]
    gt = {"images": [], "annotations": [], "categories": cats}
    rng = np.random.default_rng(5)
    store = {}
    for k, im in enumerate(imgs):
        iid = 100 + 3 * k
        name = "img%03d.jpg" % k
        store[name] = im
        gt["images"].append({"id": iid, "file_name": name, "height": im.shape[0], "width": im.shape[1]})
        for row in coco_eval.detection_records(det, im, iid, coco_eval.integer_to_coco_id(cats), 0.0):
            x, y, w, h = (float(v) + float(rng.normal(0, 2)) for v in row["bbox"])
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": iid, "category_id": row["category_id"],
                                      "bbox": [x, y, max(w, 1.0), max(h, 1.0)], "area": max(w, 1.0) * max(h, 1.0) * 40,
                                      "iscrowd": int(rng.random() < 0.15)})
    return gt, store


def test_coco_eval_sharded_gloo_equals_one_process(tmp_path):
    from ssd_amd import coco_eval
    gt, store = _coco_case()
    one = coco_eval.evaluate(sharding_stub.StubDetector(T=7), gt, "", read_image=store.__getitem__,
                             predictions_json=str(tmp_path / "pred_w1.json"), max_batch=4, read_workers=2)
    assert one[0] > 0
    det, mapping = sharding_stub.StubDetector(T=7), coco_eval.integer_to_coco_id(gt["categories"])
    rows = [r for m in sorted(gt["images"], key=lambda m: m["id"])
            for r in coco_eval.detection_records(det, store[m["file_name"]], m["id"], mapping, 0.15)]
    assert (tmp_path / "pred_w1.json").read_bytes() == json.dumps(rows).encode()
    for world in (2, 3):
        per_rank = _spawn(world, str(tmp_path))
        for stats in per_rank:
            assert np.array_equal(stats, one), (world, stats, one)
        assert (tmp_path / ("pred_w%d.json" % world)).read_bytes() == (tmp_path / "pred_w1.json").read_bytes()


# ----------------------------------------------------------------------------- CocoBoxEval subset + merge
def _synthetic_split(seed):
    rng = np.random.default_rng(seed)
    n_img, cats = 24, [1, 2, 5, 7, 9]
    gt = {"images": [{"id": 10 + i} for i in range(n_img)], "annotations": [], "categories": [{"id": c} for c in cats]}
    res = []
    for i in range(n_img):
        iid = 10 + i
        # category 9 only on the first images (one subset), category 7 only on the last ones
        allowed = [c for c in cats if not (c == 9 and i >= 6) and not (c == 7 and i < n_img - 5)]
        for _ in range(int(rng.integers(0, 7))):
            side = float(rng.choice([8.0, 20.0, 50.0, 90.0, 150.0, 300.0]))     # every area range
            x, y = rng.uniform(0, 400, 2)
            w, h = side * rng.uniform(0.6, 1.4), side * rng.uniform(0.6, 1.4)
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": iid, "category_id": int(rng.choice(allowed)),
                                      "bbox": [x, y, w, h], "area": w * h, "iscrowd": int(rng.random() < 0.12)})
        if i % 5 == 3:
            continue                                        # an image without detections
        for a in [a for a in gt["annotations"] if a["image_id"] == iid]:
            for _ in range(int(rng.integers(0, 3))):
                x, y, w, h = (v + rng.normal(0, 0.15 * a["bbox"][2]) for v in a["bbox"])
                res.append({"image_id": iid, "category_id": a["category_id"], "bbox": [x, y, abs(w) + 1, abs(h) + 1],
                            "score": float(np.round(rng.random(), 2))})           # ties in score
        for _ in range(int(rng.integers(0, 4))):                                  # false positives, any category
            res.append({"image_id": iid, "category_id": int(rng.choice(allowed)),
                        "bbox": list(rng.uniform(0, 300, 2)) + list(rng.uniform(3, 200, 2)), "score": float(rng.random())})
    return gt, res


@pytest.mark.parametrize("parts", [2, 3, 5])
def test_coco_box_eval_subsets_merge_to_one_shot(ssd, parts):
    from ssd_amd import coco_metric
    for seed in (0, 1, 2):
        gt, res = _synthetic_split(seed)
        want = coco_metric.evaluate_boxes(gt, res)
        ids = [im["id"] for im in gt["images"]]
        subsets = [ids[k::parts] for k in range(parts)]
        subsets[0] = subsets[0] + subsets[-1][:2]
        subsets[-1] = subsets[-1][2:]
        cells = []
        for sub in subsets:
            mine = [r for r in res if r["image_id"] in set(sub)]
            ev = coco_metric.CocoBoxEval(gt, mine).evaluate(img_ids=sub)
            cells.append(pickle.loads(pickle.dumps(ev.cells())))          # as they travel between processes
        merged = coco_metric.CocoBoxEval(gt, [r for r in res if r["image_id"] in set(subsets[0])]).evaluate(img_ids=subsets[0])
        for c in cells[1:]:
            merged.merge(c)
        got = merged.accumulate().summarize()
        one = coco_metric.CocoBoxEval(gt, res).evaluate().accumulate()
        assert np.array_equal(got, want), (seed, got, want)
        assert np.array_equal(merged.precision, one.precision) and np.array_equal(merged.recall, one.recall)
        assert want[0] > 0 and min(want[3:6]) > -1          # AP away from 0, every area range populated
        with pytest.raises(ValueError):
            merged.merge(cells[1])                           # a cell twice
    out = io.StringIO()
    coco_metric.CocoBoxEval(gt, res).evaluate(img_ids=[]).summarize(out)     # an empty subset is a valid share
    with pytest.raises(ValueError):
        coco_metric.CocoBoxEval(gt, res).evaluate(img_ids=[123456])
