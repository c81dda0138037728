"""Child process of tests/test_gpu_sharding.py: one rank (or the one-process run) of a sharded detection / evaluation.
    python sharding_gpu_worker.py TASK WORKDIR
The rank comes from RANK / WORLD_SIZE (set by the test, or by torch.distributed.run for task 'rccl'); results go to
WORKDIR as JSON / .npy files and the exit status says whether the in-process comparisons held."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import ssd_amd  # noqa: E402
import ssd_amd.evaluation  # noqa: E402,F401

PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15, "iou_threshold": 0.6,
          "max_boxes_per_class": 25, "min_dimension": 128}
LOSS = {"gamma": 2.0, "alpha": 0.25, "localization_loss_weight": 1.0, "classification_loss_weight": 2.0, "weight_decay": 5e-5}
SIZES = [(128, 128), (100, 150), (160, 120), (128, 256), (90, 200), (200, 130), (64, 300), (140, 141), (300, 90), (129, 128)]


def detector(num_classes=80):
    params = dict(PARAMS, num_classes=num_classes)
    W = ssd_amd.synthetic_weights(params, seed=3, logits_bias=-3.0)
    det = ssd_amd.Detector(W, config=dict(params, **LOSS), precision="f32")
    det.engine.set_option("plan_cache_mb", 256)      # two ranks share one GPU
    return det


def images(n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, SIZES[k % len(SIZES)] + (3,), dtype=np.uint8) for k in range(n)]


def init_gloo():
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    return dist.get_rank(), dist.get_world_size()


def same(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and np.array_equal(u, v) for x, y in zip(a, b) for u, v in zip(x, y))


def main(task, work):
    if task in ("detect", "rccl"):
        if task == "rccl":
            device, backend = ssd_amd.init_node_process_group()
            assert backend == "nccl" and dist.get_world_size() == 1, backend
            rank, world = 0, 1
        else:
            rank, world = init_gloo()
        det = detector()
        every = images(37, seed=1)
        split = [0, 23, 37] if world == 2 else [0, 37]            # uneven: 23 + 14
        mine = every[split[rank]:split[rank + 1]]
        got = ssd_amd.detect_many_sharded(det, mine, score_threshold=0.15, max_batch=8, chunk=9)
        if task == "rccl":
            assert ssd_amd.distributed._mixed_buffers and all(b.is_cuda for b in ssd_amd.distributed._mixed_buffers.values())
        want = det.detect_many(every, score_threshold=0.15, max_batch=32)
        assert sum(len(w[2]) for w in want) > 0
        assert same(got, want), "sharded detections differ from detect_many"
    elif task == "coco1":
        det = detector()
        imgs = json.load(open(os.path.join(work, "images.json")))
        gt = {"images": imgs, "annotations": [], "categories": [{"id": 2 * k + 1, "name": n} for k, n in enumerate(ssd_amd.coco_eval.COCO_NAMES)]}
        ssd_amd.coco_eval.evaluate(det, gt, work, predictions_json=os.path.join(work, "seed.json"), max_batch=8)
        rng = np.random.default_rng(9)
        for k, r in enumerate(json.load(open(os.path.join(work, "seed.json")))):
            if rng.random() < 0.3:
                continue                                               # a missed detection
            x, y, w, h = (float(v) + float(rng.normal(0, 1.5)) for v in r["bbox"])
            w, h = max(w, 1.0), max(h, 1.0)
            area = [w * h, 500.0, 5000.0, 20000.0][k % 4]            # all three area ranges
            gt["annotations"].append({"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": [x, y, w, h],
                                      "area": area, "iscrowd": int(rng.random() < 0.1)})
        json.dump(gt, open(os.path.join(work, "gt.json"), "w"))
        stats = ssd_amd.coco_eval.evaluate(det, gt, work, predictions_json=os.path.join(work, "pred_1.json"), max_batch=8)
        np.save(os.path.join(work, "stats_1.npy"), stats)
        assert stats[0] > 0, stats
    elif task == "coco2":
        rank, world = init_gloo()
        det = detector()
        gt = json.load(open(os.path.join(work, "gt.json")))
        stats = ssd_amd.coco_eval.evaluate(det, gt, work, predictions_json=os.path.join(work, "pred_2.json"), max_batch=8,
                                           group=dist.group.WORLD, chunk=4)
        np.save(os.path.join(work, "stats_2_rank%d.npy" % rank), stats)
    elif task in ("eval1", "eval2"):
        group, chunk, rank = None, 256, 0
        if task == "eval2":
            rank, _world = init_gloo()
            group, chunk = dist.group.WORLD, 3
        det = detector(num_classes=3)
        res = ssd_amd.evaluation.evaluate(det, os.path.join(work, "shard"), dict(PARAMS, num_classes=3, **LOSS), max_batch=4, group=group, chunk=chunk)
        json.dump(res, open(os.path.join(work, "%s_rank%d.json" % (task, rank)), "w"), sort_keys=True)
    else:
        raise SystemExit("unknown task " + task)
    if dist.is_initialized():
        dist.destroy_process_group()
    print("worker ok", task)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
