"""What train.py's evaluation metric costs on the host and on the GPU, in ONE process on coco_metric_cost.py's
synthetic val2017-sized set:

    python scripts/voc_metric_cost.py [--images 5000] [--rounds 3]

  the set      coco_metric_cost.result_set: `--images` images, 80 labels, about 7 groundtruth boxes and 25 detections per image; the
               xywh boxes become (ymin, xmin, ymax, xmax), the category ids labels 0..79, one add_image per image.
  the timings  coco_eval.Evaluator: add_image of every image, evaluate().  voc_match.VocEvaluator: add_image of every image,
               evaluate(device=0) end to end and split into pack (numpy), upload, the two launches (HIP events), download and the
               dict.  `--rounds` rounds, host and GPU alternating, the median.  The curve kernel's serial chain -- dependent float64
               additions over the rows of the longest label -- is measured on its own: ssd_voc_curve on that one segment.
  the check    in every round the two dicts agree as tests/test_voc_match_host.py asks: six values per label equal, AP within
               2 * tp * 2^-53.
There is no speed gate: the log says what each part costs, whichever way it comes out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import coco_eval, voc_match                          # noqa: E402
from coco_metric_cost import K, result_set                        # noqa: E402

EXACT = ("precision", "recall", "best_threshold", "mean_iou_for_TP", "total_FP", "total_FN")


def per_image(gt, dets):
    """the COCO-style dicts -> add_image's five arrays per image"""
    rows = {im["id"]: ([], [], [], [], []) for im in gt["images"]}
    for a in gt["annotations"]:
        x, y, w, h = a["bbox"]
        rows[a["image_id"]][0].append([y, x, y + h, x + w])
        rows[a["image_id"]][1].append(a["category_id"] - 1)
    for d in dets:
        x, y, w, h = d["bbox"]
        r = rows[d["image_id"]]
        r[2].append([y, x, y + h, x + w])
        r[3].append(d["category_id"] - 1)
        r[4].append(d["score"])
    return [(np.array(r[0], np.float32).reshape(-1, 4), np.array(r[1], np.int64), np.array(r[2], np.float32).reshape(-1, 4),
             np.array(r[3], np.int64), np.array(r[4], np.float32)) for r in rows.values()]


def check(got, want, rows):
    worst = 0.0
    for label in range(K):
        for k in EXACT:
            assert got[label][k] == want[label][k], (label, k, got[label][k], want[label][k])
        bound = 2.0 * (rows[label] - want[label]["total_FP"]) * 2.0 ** -53
        assert abs(got[label]["AP"] - want[label]["AP"]) <= bound, (label, got[label]["AP"], want[label]["AP"])
        worst = max(worst, abs(got[label]["AP"] - want[label]["AP"]) / bound if bound else 0.0)
    return worst


def longest_chain(ev, rounds):
    """ssd_voc_curve on the longest label's segment alone -> (its rows, seconds by HIP events, the median)"""
    p = voc_match.pack(ev.num_classes, *ev._flat())
    _res, tp, tp_iou = voc_match.evaluate_packed(p, 0.5, 0, want_rows=True)
    seg = p["segments"][int(np.argmax(p["segments"]["count"])):][:1].copy()
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tp, tp_iou, conf, seg_dev = up(tp), up(tp_iou), up(p["conf"]), up(seg.view(np.uint8).reshape(-1))
    out = torch.empty(64, dtype=torch.uint8, device=dev)
    times = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        voc_match.launch(None, None, None, None, 0, None, 0, 0.5, tp, tp_iou, p["n_rows"], seg, seg_dev, conf, out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return int(seg["count"][0]), float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0))
    images = per_image(*result_set(args.images))
    rows = np.bincount(np.concatenate([im[3] for im in images]), minlength=K).tolist()
    warm = voc_match.VocEvaluator(K)                                 # loads the library, creates the context
    warm.add_image(*images[0])
    warm.evaluate(device=0)
    host_add, host_eval, gpu_add, gpu_eval, parts, worst = [], [], [], [], [], 0.0
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        host = coco_eval.Evaluator(K)
        for im in images:
            host.add_image(*im)
        t1 = time.perf_counter()
        want = host.evaluate()
        t2 = time.perf_counter()
        ev = voc_match.VocEvaluator(K)
        for im in images:
            ev.add_image(*im)
        t3 = time.perf_counter()
        timings = {}
        got = ev.evaluate(device=0, timings=timings)
        t4 = time.perf_counter()
        host_add.append(t1 - t0), host_eval.append(t2 - t1), gpu_add.append(t3 - t2), gpu_eval.append(t4 - t3), parts.append(timings)
        worst = max(worst, check(got, want, rows))
        assert abs(got["mAP"] - want["mAP"]) <= 2.0 ** -40
    n_chain, t_chain = longest_chain(ev, args.rounds)
    p = voc_match.pack(K, *ev._flat())
    med = lambda xs: float(np.median(xs))
    print("images %d, labels %d, groundtruth boxes %d, detections %d, cells %d (max D %d, max G %d), longest label %d rows"
          % (len(images), K, len(p["gt_box"]), p["n_rows"], len(p["cells"]), p["cells"]["D"].max(), p["cells"]["G"].max(), n_chain))
    print("the two dicts agree in every round (%d rounds): six values per label equal, worst |AP - host AP| = %.4f of 2 tp 2^-53; mAP %.6f"
          % (args.rounds, worst, got["mAP"]))
    show = lambda name, xs: print("%-44s %8.4f s   (rounds: %s)" % (name, med(xs), " ".join("%.4f" % x for x in xs)))
    show("Evaluator.add_image, all images", host_add)
    show("Evaluator.evaluate()", host_eval)
    show("VocEvaluator.add_image, all images", gpu_add)
    show("VocEvaluator.evaluate(device=0), end to end", gpu_eval)
    for k, note in (("pack", "numpy, on the host"), ("upload", ""), ("match", "HIP events"), ("curve", "HIP events"), ("download", ""),
                    ("dict", "Python, on the host")):
        print("    %-40s %8.5f s   %s" % (k, med([q[k] for q in parts]), note))
    print("%-44s %8.5f s   (%d rows, one wave: %.1f ns per row)" % ("ssd_voc_curve, the longest label alone", t_chain, n_chain,
                                                                     t_chain / max(n_chain, 1) * 1e9))
    h, g = med(host_add) + med(host_eval), med(gpu_add) + med(gpu_eval)
    print("add_image + evaluate: host %.3f s, GPU path %.3f s: host / GPU path = %.2fx" % (h, g, h / g))


if __name__ == "__main__":
    main()
