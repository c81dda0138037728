"""What tiled detection costs, in ONE process on ONE synthetic 1200 x 1600 frame, config_mobilenet.json
(min_dimension 640: nine 640 x 640 tiles at overlap 0.25, plus the whole frame as 640 x 896), synthetic weights:

    python scripts/tiled_cost.py [--rounds 20] [--log FILE]

  the parts    HIP events around each device step of Detector.detect_tiled, as it makes them: the gather, the tiles' forwards
               (9 tiles as batches of 8 + 1), the whole frame's forward, the merge.  `--rounds` rounds, the median.  The gather is
               one short launch, so it is timed a second time as 50 launches between one event pair.
  the wall     Detector.detect_tiled(frame) from a host frame to host results, against the hand-made path on the API without it:
               numpy crops, detect_batch(crops), detect_batch(frame), the reference merge of tests/helpers/tile_ref.py (numpy + the
               oracle's NMS) and the score filter.  Alternating, `--rounds` rounds, the median and the spread.
  the check    both paths return the same boxes, labels and scores, bit for bit.
There is no speed gate: the log says what each part costs, whichever way it comes out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd.ssd import pack_records, score_filter                # noqa: E402
from oracle import ops                                            # noqa: E402
from helpers import tile_ref as ref                               # noqa: E402

H, W, OVERLAP = 1200, 1600, 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ops.build()
    params = ssd_amd.load_config(os.path.join(ROOT, "tests", "golden", "config_mobilenet.json"))
    det = ssd_amd.Detector(ssd_amd.synthetic_weights(params, seed=1, logits_bias=-4.0), config=params)
    eng = det.engine
    md, C, m, thr = params["min_dimension"], params["num_classes"], params["max_boxes_per_class"], params["iou_threshold"]
    rng = np.random.default_rng(2)
    coarse = rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)
    frame = np.ascontiguousarray(np.repeat(np.repeat(coarse, 16, 0), 16, 1))
    ys, xs = ssd_amd.tile_grid(H, W, md, md, OVERLAP)
    n = len(ys) * len(xs)
    say("device: %s, precision %s" % (torch.cuda.get_device_name(0), eng.precision))
    say("frame %d x %d, tile %d, overlap %.2f: rows %s, columns %s, %d tiles; whole frame as %s; C %d, m %d"
        % (H, W, md, OVERLAP, ys, xs, n, eng.network_shape(H, W), C, m))

    def by_hand(parts=None):
        t0 = time.perf_counter()
        crops = ref.crops(frame[None], md, md, OVERLAP)
        t1 = time.perf_counter()
        tile_rec = pack_records(*det.detect_batch(crops))
        full_rec = pack_records(*det.detect_batch(frame[None]))
        t2 = time.perf_counter()
        boxes, labels, scores, num = ref.split(ref.merge(ops, tile_rec, full_rec, 1, H, W, md, md, OVERLAP, C, m, thr))
        out = score_filter(boxes[0], labels[0], scores[0], num[0], 0.1)
        t3 = time.perf_counter()
        if parts is not None:
            parts.append((t1 - t0, t2 - t1, t3 - t2))
        return out

    # ---- warm up every shape and both paths; the check
    for _ in range(3):
        got = det.detect_tiled(frame)
        want = by_hand()
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    say("detect_tiled and the hand-made path return the same %d boxes, bit for bit" % len(got[2]))

    # ---- the device steps between HIP events, as detect_tiled enqueues them
    dev = torch.from_numpy(frame).cuda().view(1, H, W, 3)
    tiles = ssd_amd.tiles.tile_gather(dev, md, md, OVERLAP)
    rec, rec_full = eng.new_records(n, "cuda:0"), eng.new_records(1, "cuda:0")
    out = eng.new_records(1, "cuda:0")
    sizes = [32, 16, 8, 4, 2, 1]

    def forwards():
        k = 0
        for b in sizes:
            while n - k >= b:
                eng.forward(tiles[k:k + b], records=rec[k:k + b])
                k += b
    steps = (("gather (ssd_tile_gather)", lambda: ssd_amd.tiles.tile_gather(dev, md, md, OVERLAP, out=tiles)),
             ("tiles' forwards (8 + 1)", forwards),
             ("whole frame's forward", lambda: eng.forward(dev, records=rec_full)),
             ("merge (ssd_tile_merge, 2 launches)", lambda: ssd_amd.tiles.tile_merge(rec, rec_full, (1, H, W), md, md, OVERLAP, C, m, thr, out=out)))
    ms = {name: [] for name, _ in steps}
    for r in range(args.rounds + 2):
        for name, fn in steps:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 2:
                ms[name].append(a.elapsed_time(b))
    say("device steps, HIP events, median of %d rounds (min .. max), ms:" % args.rounds)
    total = 0.0
    for name, _ in steps:
        v = np.array(ms[name])
        total += float(np.median(v))
        say("    %-36s %8.3f   (%.3f .. %.3f)" % (name, np.median(v), v.min(), v.max()))
    say("    %-36s %8.3f" % ("sum of the medians", total))
    # one short launch between an event pair is close to the events' resolution: the gather again as 50 launches back to back
    per = []
    for r in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            ssd_amd.tiles.tile_gather(dev, md, md, OVERLAP, out=tiles)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / 50)
    per = np.array(per)
    moved = frame.nbytes + tiles.numel()
    say("    %-36s %8.4f   (%.4f .. %.4f) per launch: %.2f TB/s over %.2f MB read + written (the frame stays in the caches)"
        % ("gather, 50 launches back to back", np.median(per), per.min(), per.max(), moved / np.median(per) / 1e9, moved / 1e6))
    nb = ref.split(rec.cpu().numpy())[3]
    say("boxes per tile %s, whole frame %d, merged %d" % (nb.tolist(), int(ref.split(rec_full.cpu().numpy())[3][0]), int(ref.split(out.cpu().numpy())[3][0])))
    say("bytes: frame %.2f MB uploaded once; tiles %.2f MB written on the device (the hand-made path uploads them: %.2f MB + the frame)"
        % (frame.nbytes / 1e6, tiles.numel() / 1e6, tiles.numel() / 1e6))

    # ---- wall time, host frame in, host results out, alternating
    tiled_s, hand_s, parts = [], [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        det.detect_tiled(frame)
        tiled_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        by_hand(parts)
        hand_s.append(time.perf_counter() - t0)
    t, h, p = np.array(tiled_s) * 1e3, np.array(hand_s) * 1e3, np.array(parts) * 1e3
    say("wall time per frame, median of %d alternating rounds (min .. max), ms:" % args.rounds)
    say("    %-36s %8.3f   (%.3f .. %.3f)" % ("Detector.detect_tiled", np.median(t), t.min(), t.max()))
    say("    %-36s %8.3f   (%.3f .. %.3f)" % ("hand-made path", np.median(h), h.min(), h.max()))
    for k, name in enumerate(("numpy crops", "two detect_batch calls", "reference merge + filter (host)")):
        say("        %-32s %8.3f" % (name, np.median(p[:, k])))
    say("hand-made / detect_tiled = %.2fx" % (np.median(h) / np.median(t)))
    det.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
