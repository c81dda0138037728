"""What the COCO metric costs on the host and with the matching and the accumulation on the GPU, in ONE
process on ONE synthetic val2017-sized result set:

    python scripts/coco_metric_cost.py [--images 5000] [--rounds 3]

  the set      `--images` images, 80 categories, 1 to 14 annotations per image (about 7) in 1 to 3 of the categories, 3 % of them
               crowd; per annotation 0 to 3 detections that are near-duplicates of its box (normal jitter, sigma 6 pixels) and per
               image 5 to 24 stray detections of any category: about 25 detections per image.
  the timings  the constructor; CocoBoxEval.evaluate() on the host; evaluate(device=0) end to end and split into pack, upload,
               launch (HIP events), download and unpack; evaluate(device=0, unpack=False); accumulate() on the host;
               accumulate(device=0) from the retained device arrays, end to end and split into pack_order, upload, launch (HIP
               events) and download, and again through the upload route (flattening eval_imgs).  `--rounds` rounds, host and GPU
               alternating, the median.
  the check    the two evaluations' cells() are equal in all seven arrays, key order included; precision and recall of every
               accumulate(device=0) equal the host's bit for bit in every round; so are the twelve statistics.
There is no speed gate: the log says what each part costs, whichever way it comes out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import coco_metric                                   # noqa: E402

K = 80


def result_set(n_images, seed=0):
    rng = np.random.default_rng(seed)
    images = [{"id": i + 1} for i in range(n_images)]
    cats = [{"id": k + 1} for k in range(K)]
    anns, dets = [], []
    for im in images:
        present = rng.choice(K, size=rng.integers(1, 4), replace=False) + 1
        for _ in range(rng.integers(1, 15)):
            w, h = rng.uniform(8, 300, 2)
            x, y = rng.uniform(0, 340, 2)
            c = int(rng.choice(present))
            anns.append({"image_id": im["id"], "category_id": c, "bbox": [float(x), float(y), float(w), float(h)], "area": float(w * h * 0.7),
                         "iscrowd": int(rng.random() < 0.03)})
            for _ in range(rng.integers(0, 4)):
                j = rng.normal(0, 6, 4)
                dets.append({"image_id": im["id"], "category_id": c, "score": float(np.float32(rng.uniform(0.15, 1))),
                             "bbox": [int(x + j[0]), int(y + j[1]), max(1, int(w + j[2])), max(1, int(h + j[3]))]})
        for _ in range(rng.integers(5, 25)):
            w, h = rng.uniform(8, 300, 2)
            x, y = rng.uniform(0, 340, 2)
            dets.append({"image_id": im["id"], "category_id": int(rng.integers(1, K + 1)), "bbox": [int(x), int(y), int(w), int(h)],
                         "score": float(np.float32(rng.uniform(0.15, 0.6)))})
    return {"images": images, "annotations": anns, "categories": cats}, dets


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0))
    gt, dets = result_set(args.images)
    t0 = time.perf_counter()
    ev = coco_metric.CocoBoxEval(gt, dets)
    t_init = time.perf_counter() - t0
    coco_metric.CocoBoxEval(gt, dets[:100]).evaluate(device=0, unpack=False).accumulate(device=0)      # loads the library, creates the context
    host_s, gpu_s, parts = [], [], []
    lazy_s, acc_host_s, acc_gpu_s, acc_parts, acc_up_s, acc_up_parts = [], [], [], [], [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        ev.evaluate()
        host_s.append(time.perf_counter() - t0)
        host_cells = ev.cells()
        t0 = time.perf_counter()
        ev.accumulate()
        acc_host_s.append(time.perf_counter() - t0)
        want_p, want_r = ev.precision, ev.recall
        ev.eval_imgs = {}
        timings = {}
        t0 = time.perf_counter()
        ev._evaluate_on_gpu(ev.img_ids, 0, timings=timings)
        gpu_s.append(time.perf_counter() - t0)
        parts.append(timings)
        gpu_cells = ev.cells()
        for k in ("keys", "D", "G", "scores", "matched", "ignored", "gt_ignore"):
            assert gpu_cells[k].dtype == host_cells[k].dtype and np.array_equal(gpu_cells[k], host_cells[k]), k
        # the upload route: eval_imgs (here the GPU matching's, unpacked) flattened on the host
        timings = {}
        t0 = time.perf_counter()
        ev._accumulate_on_gpu(0, timings=timings)
        acc_up_s.append(time.perf_counter() - t0)
        acc_up_parts.append(timings)
        assert timings["route"] == "upload" and same_bits(ev.precision, want_p) and same_bits(ev.recall, want_r)
        # the retained route: nothing unpacked, the matching's outputs stay on the GPU
        t0 = time.perf_counter()
        ev.evaluate(device=0, unpack=False)
        torch.cuda.synchronize()
        lazy_s.append(time.perf_counter() - t0)
        timings = {}
        t0 = time.perf_counter()
        ev._accumulate_on_gpu(0, timings=timings)
        acc_gpu_s.append(time.perf_counter() - t0)
        acc_parts.append(timings)
        assert timings["route"] == "retained" and "eval_imgs" not in ev.__dict__
        assert same_bits(ev.precision, want_p) and same_bits(ev.recall, want_r)
    stats_gpu = ev.summarize()
    stats_host = coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate().summarize()
    assert all(float(a) == float(b) for a, b in zip(stats_gpu, stats_host))
    c = host_cells
    n_cells = len(c["D"]) // len(coco_metric.AREA_RNG)
    print("images %d, categories %d, annotations %d, detections %d, cells %d, kept detections %d, max D %d, max G %d"
          % (args.images, K, len(gt["annotations"]), len(dets), n_cells, c["D"].sum() // len(coco_metric.AREA_RNG), c["D"].max(), c["G"].max()))
    print("the two cells() are equal in all seven arrays, precision and recall of accumulate(device=0) equal the host's bit for bit on both "
          "routes, and the twelve statistics are equal (%d rounds); AP %.4f" % (args.rounds, stats_gpu[0]))
    med = lambda xs: float(np.median(xs))
    print("%-34s %8.3f s" % ("constructor", t_init))
    print("%-34s %8.3f s   (rounds: %s)" % ("evaluate(), host loop", med(host_s), " ".join("%.3f" % x for x in host_s)))
    print("%-34s %8.3f s   (rounds: %s)" % ("evaluate(device=0), end to end", med(gpu_s), " ".join("%.3f" % x for x in gpu_s)))
    for k in ("pack", "upload", "launch", "download", "unpack"):
        print("    %-30s %8.4f s" % (k + (" (HIP events)" if k == "launch" else ""), med([p[k] for p in parts])))
    print("%-34s %8.3f s   (rounds: %s)" % ("evaluate(device=0, unpack=False)", med(lazy_s), " ".join("%.3f" % x for x in lazy_s)))
    print("%-34s %8.3f s   (rounds: %s)" % ("accumulate(), host loop", med(acc_host_s), " ".join("%.3f" % x for x in acc_host_s)))
    for name, total, split in (("accumulate(device=0), retained", acc_gpu_s, acc_parts), ("accumulate(device=0), upload route", acc_up_s, acc_up_parts)):
        print("%-34s %8.3f s   (rounds: %s)" % (name, med(total), " ".join("%.3f" % x for x in total)))
        for k in ("pack_order", "upload", "launch", "download"):
            label = {"pack_order": "pack_order" if split is acc_parts else "cells() + pack_cells", "launch": "launch (HIP events)"}.get(k, k)
            print("    %-30s %8.4f s" % (label, med([p[k] for p in split])))
    print("evaluate: host / GPU path = %.2fx; accumulate: host / GPU path = %.2fx (retained), %.2fx (upload route)"
          % (med(host_s) / med(gpu_s), med(acc_host_s) / med(acc_gpu_s), med(acc_host_s) / med(acc_up_s)))
    print("the metric: constructor %.2f s + evaluate %.2f s + accumulate %.2f s on the host; %.2f + %.2f + %.2f s with unpacking and the "
          "host accumulate(); %.2f + %.2f + %.2f s with unpack=False and accumulate(device=0)"
          % (t_init, med(host_s), med(acc_host_s), t_init, med(gpu_s), med(acc_host_s), t_init, med(lazy_s), med(acc_gpu_s)))


if __name__ == "__main__":
    main()
