"""What the COCO metric costs from the detector's records, through the result dicts and without them, in ONE process
on ONE synthetic val2017-sized result set:

    python scripts/coco_rows_cost.py [--images 5000] [--rounds 3] [--log profiles/coco_rows_cost.log]

  the set      coco_metric_cost.result_set (`--images` images, 80 categories, about 25 detections per image), held the way the
               engine leaves it: one unfiltered record of T = 2000 rows per image in a device block, every image 1024 x 1024 (a
               power of two, so the records' normalised boxes give back the set's integer boxes).
  the routes   both with the matching and the accumulation on the GPU (metric_device = 0), both starting from the device block:
               dicts    the block downloaded, coco_eval.detection_records_many's row building (a stub detector that filters the
                        downloaded records), the CocoBoxEval constructor, evaluate(device=0, unpack=False), accumulate(device=0);
               records  CocoBoxEval.from_records(device=0), the same two calls -- split into the groundtruth side of the
                        constructor, count / scan / fill (HIP events), the downloads, the cell table, the matching.
               `--rounds` rounds, the routes alternating, the median.  gc.collect() runs, untimed, in front of every timed
               route: a full collection over the other route's 130 000 live containers costs 0.25 s wherever it happens to fall,
               and without this it falls into whichever call crosses the allocation count.  What a route's own allocations
               trigger stays in its time.
  the check    the two routes' precision and recall are equal bit for bit in every round, and so are the twelve statistics.
There is no speed gate: the log says what each part costs, whichever way it comes out."""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import coco_eval, coco_metric, coco_rows             # noqa: E402
from ssd_amd.ssd import score_filter, split_records               # noqa: E402
from coco_metric_cost import K, result_set, same_bits             # noqa: E402

T, SIDE, THR = 2000, 1024, 0.15


def as_records(gt, dets):
    ids = [im["id"] for im in gt["images"]]
    at = {i: k for k, i in enumerate(ids)}
    rec = np.zeros((len(ids), 6 * T + 1), np.int32)
    boxes, labels, scores, num = split_records(rec)
    for d in dets:
        i = at[d["image_id"]]
        x, y, w, h = d["bbox"]
        boxes[i, num[i]] = [y / SIDE, x / SIDE, (y + h) / SIDE, (x + w) / SIDE]
        labels[i, num[i]] = d["category_id"] - 1
        scores[i, num[i]] = d["score"]
        num[i] += 1
    return rec, ids


class Downloaded:
    """detect_many of a detector whose batches are already computed: the score filter over the downloaded records"""

    def __init__(self, rec):
        self.rec = rec

    def detect_many(self, images, score_threshold, max_batch):
        return [score_filter(b, l, s, n, score_threshold) for b, l, s, n in zip(*split_records(self.rec))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "coco_rows_cost.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("device: %s" % torch.cuda.get_device_name(0))
    gt, dets = result_set(args.images)
    gt = dict(gt, images=[dict(im, height=SIDE, width=SIDE) for im in gt["images"]])
    rec_host, ids = as_records(gt, dets)
    mapping = {k: k + 1 for k in range(K)}
    frames = [np.empty((SIDE, SIDE, 0), np.uint8)] * len(ids)
    records = torch.from_numpy(rec_host).cuda()
    coco_metric.CocoBoxEval.from_records(gt, records[:8], ids[:8], mapping, THR, device=0).evaluate(device=0, unpack=False).accumulate(device=0)
    med = lambda xs: float(np.median(xs))
    dict_s, rec_s = {k: [] for k in ("download", "rows", "constructor", "evaluate", "accumulate", "total")}, \
        {k: [] for k in ("from_records", "evaluate", "accumulate", "total")}
    parts = {k: [] for k in ("groundtruth", "count", "scan", "fill", "download", "cells", "match")}
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        gc.collect()
        t0 = time.perf_counter()
        host = records.cpu().numpy()
        t1 = time.perf_counter()
        rows = coco_eval.detection_records_many(Downloaded(host), frames, ids, mapping, THR)
        t2 = time.perf_counter()
        a = coco_metric.CocoBoxEval(gt, rows)
        t3 = time.perf_counter()
        a.evaluate(device=0, unpack=False)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        a.accumulate(device=0)
        t5 = time.perf_counter()
        for k, v in zip(("download", "rows", "constructor", "evaluate", "accumulate", "total"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t5 - t0)):
            dict_s[k].append(v)
        n_rows = len(rows)
        del rows, host

        gc.collect()
        t0 = time.perf_counter()
        b = coco_metric.CocoBoxEval.from_records(gt, records, ids, mapping, THR, device=0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        b.evaluate(device=0, unpack=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        b.accumulate(device=0)
        t3 = time.perf_counter()
        for k, v in zip(("from_records", "evaluate", "accumulate", "total"), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
            rec_s[k].append(v)
        assert "eval_imgs" not in b.__dict__ and b._dts is None
        assert same_bits(a.precision, b.precision) and same_bits(a.recall, b.recall)
        assert all(float(x) == float(y) for x, y in zip(a.summarize(), b.summarize()))

        # the records route's parts, each timed on its own
        gc.collect()
        t0 = time.perf_counter()
        coco_metric.CocoBoxEval(gt, [])
        parts["groundtruth"].append(time.perf_counter() - t0)
        tm = {}
        l2c = np.arange(K, dtype=np.int32)
        coco_rows.rows_device(records, np.full((len(ids), 2), SIDE, np.int32), l2c, K, THR, 0, timings=tm)
        for k in ("count", "scan", "fill", "download"):
            parts[k].append(tm[k])
        tm = {}
        c = coco_metric.CocoBoxEval.from_records(gt, records, ids, mapping, THR, device=0)
        c._evaluate_on_gpu(c.img_ids, 0, timings=tm, unpack=False)
        parts["cells"].append(tm["pack"])
        parts["match"].append(tm["upload"] + tm["launch"])
    say("images %d, categories %d, annotations %d, detections %d (rows above %.2f: %d), record rows T %d, the block %.0f MB"
        % (args.images, K, len(gt["annotations"]), len(dets), THR, n_rows, T, rec_host.nbytes / 1e6))
    say("precision, recall and the twelve statistics of the two routes are equal bit for bit (%d rounds); AP %.4f" % (args.rounds, b.stats[0]))
    rounds = lambda xs: " ".join("%.3f" % x for x in xs)
    say("%-44s %8.3f s   (rounds: %s)" % ("dicts: records -> statistics' arrays", med(dict_s["total"]), rounds(dict_s["total"])))
    for k, label in (("download", "download of the block"), ("rows", "detection_records_many's rows"), ("constructor", "CocoBoxEval(gt, rows)"),
                     ("evaluate", "evaluate(device=0, unpack=False)"), ("accumulate", "accumulate(device=0)")):
        say("    %-40s %8.4f s" % (label, med(dict_s[k])))
    say("%-44s %8.3f s   (rounds: %s)" % ("records: records -> statistics' arrays", med(rec_s["total"]), rounds(rec_s["total"])))
    for k, label in (("from_records", "from_records(device=0)"), ("evaluate", "evaluate(device=0, unpack=False)"), ("accumulate", "accumulate(device=0)")):
        say("    %-40s %8.4f s" % (label, med(rec_s[k])))
    say("  the records route's parts, timed on their own:")
    for k, label in (("groundtruth", "the constructor's groundtruth side"), ("count", "count (HIP events)"), ("scan", "scan (HIP events)"),
                     ("fill", "fill (HIP events)"), ("download", "downloads: counts, bad, det_score"), ("cells", "the cell table (with pack of the groundtruth)"),
                     ("match", "upload of the groundtruth + matching launch")):
        say("    %-48s %9.3f ms" % (label, med(parts[k]) * 1e3))
    say("dicts / records = %.2fx" % (med(dict_s["total"]) / med(rec_s["total"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
