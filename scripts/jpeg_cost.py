"""What decoding JPEGs on the GPU costs, part by part and end to end, on the synthetic val2017-like folder of
scripts/eval_from_disk.py (JPEGs of the 13 COCO-typical sizes, 480 x 640 class, 4:2:0, quality 90):

    python scripts/jpeg_cost.py [--images 1040] [--rounds 3] [--parent DIR] [--log profiles/jpeg_decode_cost.log]
    python scripts/jpeg_cost.py --tree DIR --folder DIR [--only rows_device] [--gc] [--label NAME] [--rounds 5]
    python scripts/jpeg_cost.py --entropy-against DIR [--images 208] [--rounds 5] [--log profiles/jpeg_loud_cost.log]

  per image    PIL decode on one core; ssd_jpeg_info_read + ssd_jpeg_entropy on one core (into pinned memory); the upload of a
               32-image batch's coefficients, tables and table rows (HIP events); ssd_jpeg_decode's two launches on that batch
               (HIP events); medians over the batches of the folder.
  end to end   coco_eval.evaluate from the files to the twelve statistics: the default route, jpeg_device=0, and both again with
               rows_device=0 -- `--rounds` rounds in ONE process, the routes alternating, the median.  Every route's statistics and
               predictions file are compared with the default route's in every round.
  --parent DIR another checkout of this repository (the commit before the decoder) with its library built: a child process of this
               script imports THAT tree and times its default and rows_device routes on the same folder, once in front of and once
               behind this tree's rounds.
  --tree DIR   the end-to-end routes of the checkout at DIR alone, in this one process, on --folder: a change and its parent commit
               timed alternately, process after process (profiles/records_route_refactor_ab.log).
  --entropy-against DIR   the host stage alone (ssd_jpeg_info_read + ssd_jpeg_entropy, one core) of this tree's library and of the
               library built in the checkout at DIR, both loaded into this ONE process and timed file by file in alternating order;
               per library the median per image of every round.  Needs no GPU.
There is no speed gate: no ratio was promised in advance, the log says what was measured, whichever way it comes out."""
import argparse
import ctypes
import gc
import json
import os
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=1040)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--log", default=None)
ap.add_argument("--tree", default=None, help="(the child's mode) time the default routes of the checkout at this path on --folder")
ap.add_argument("--folder", default=None, help="(the child's mode) the folder; written first when it holds no instances.json")
ap.add_argument("--only", default=None, help="(the child's mode) all four routes whose name contains this, not the two default ones")
ap.add_argument("--gc", action="store_true", help="(the child's mode) an untimed gc.collect() in front of every timed route")
ap.add_argument("--label", default="parent", help="(the child's mode) what the printed lines begin with")
ap.add_argument("--entropy-against", default=None, help="time the host stage of this tree and of the checkout at this path alternately")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np            # noqa: E402
import torch                  # noqa: E402
import ssd_amd                # noqa: E402
import bench                  # noqa: E402
from PIL import Image         # noqa: E402

P = bench.PARAMS
med = lambda xs: float(np.median(xs))


def write_folder(d, n):
    """eval_from_disk.py's folder: smooth scenes with a little texture, compressing like photographs."""
    rng = np.random.default_rng(0)
    order = rng.permutation(np.repeat(np.arange(len(bench.MIXED_SIZES)), -(-n // len(bench.MIXED_SIZES))))[:n]
    images, anns = [], []
    for k, i in enumerate(order):
        h, w = bench.MIXED_SIZES[i]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        base = np.stack([127 + 100 * np.sin(xx / (20 + 3 * c) + k) * np.cos(yy / (25 + 2 * c)) for c in range(3)], -1)
        im = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        name = "%012d.jpg" % (k + 1)
        Image.fromarray(im).save(os.path.join(d, name), quality=90)
        images.append({"id": k + 1, "file_name": name, "height": h, "width": w})
        anns.append({"id": k + 1, "image_id": k + 1, "category_id": 1, "bbox": [10, 10, w // 3, h // 3], "area": float((w // 3) * (h // 3)), "iscrowd": 0})
    cats = [{"id": i + 1 + (i > 10), "name": nm} for i, nm in enumerate(ssd_amd.coco_eval.COCO_NAMES)]
    gt = {"images": images, "annotations": anns, "categories": cats}
    with open(os.path.join(d, "instances.json"), "w") as f:
        json.dump(gt, f)
    return gt


def harness(det, gt, d, routes, rounds, say, label):
    """{route: [seconds per round]}; every route against the first one's statistics and file."""
    times = {name: [] for name, _kw in routes}
    for name, kw in routes:                                     # builds the plans, grows the buffers
        ssd_amd.coco_eval.evaluate(det, gt, d, predictions_json=None, **kw)
    n = len(gt["images"])
    for r in range(rounds):
        want = None
        for name, kw in (routes if r % 2 == 0 else routes[::-1]):
            path = os.path.join(d, "pred_%s.json" % name.replace(" ", "_"))
            if args.gc:                                         # (a full collection then never falls into a timed route)
                gc.collect()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ssd_amd.coco_eval.evaluate(det, gt, d, predictions_json=path, **kw)
            times[name].append(time.perf_counter() - t0)
            got = ([float(x) for x in st], open(path, "rb").read())
            if want is None:
                want = got
            assert got == want, "route %s differs from the first route of the round" % name
    for name, _kw in routes:
        say("  %-12s %-34s %7.3f s = %5.0f img/s   (rounds: %s)" % (label, name, med(times[name]), n / med(times[name]),
                                                                   " ".join("%.3f" % t for t in times[name])))
    return times


ROUTES = [("default", {}), ("jpeg_device=0", {"jpeg_device": 0}), ("rows_device=0", {"rows_device": 0}),
          ("jpeg_device=0, rows_device=0", {"jpeg_device": 0, "rows_device": 0})]


def child():
    """The checkout at --tree on the folder, one fresh process: its default and rows_device routes (the lines the parent process
    relays), or with --only every route of that name -- two trees timed alternately, run after run, on one folder."""
    if not os.path.exists(os.path.join(args.folder, "instances.json")):
        os.makedirs(args.folder, exist_ok=True)
        write_folder(args.folder, args.images)
    gt = json.load(open(os.path.join(args.folder, "instances.json")))
    det = ssd_amd.Detector(ssd_amd.synthetic_weights(P, seed=0, logits_bias=-7.5), config=P)
    routes = [r for r in ROUTES if args.only in r[0]] if args.only else [ROUTES[0], ROUTES[2]]
    harness(det, gt, args.folder, routes, args.rounds, lambda s: print(s, flush=True), args.label + (" gc" if args.gc else ""))


def entropy_ab(say):
    """The host stage of two builds on the same files, alternating file by file in one process."""
    from ssd_amd._lib import SsdJpegInfo, lib_path
    other = os.path.join(os.path.abspath(args.entropy_against), os.path.relpath(lib_path(), ROOT))
    libs = []
    for label, path in (("this tree", lib_path()), ("other tree", other)):
        L = ctypes.CDLL(path)
        L.ssd_jpeg_info_read.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p]
        L.ssd_jpeg_entropy.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        libs.append((label, L))
    d = tempfile.mkdtemp(prefix="val_like_")
    gt = write_folder(d, args.images)
    blobs = [open(os.path.join(d, m["file_name"]), "rb").read() for m in gt["images"]]
    say("%d JPEGs, %.0f KB each; ssd_jpeg_info_read + ssd_jpeg_entropy, one core, ms per image (median over the files of a round)"
        % (len(blobs), sum(map(len, blobs)) / 1024 / len(blobs)))
    out = np.empty(32 << 20, np.int16)
    rounds = {label: [] for label, _L in libs}
    for r in range(args.rounds + 1):                            # (round 0 warms both up and is not reported)
        times = {label: [] for label, _L in libs}
        for i, b in enumerate(blobs):
            for label, L in (libs if (r + i) % 2 == 0 else libs[::-1]):
                info = SsdJpegInfo()
                t0 = time.perf_counter()
                rc = L.ssd_jpeg_info_read(b, len(b), ctypes.byref(info))
                if rc == 0:
                    rc = L.ssd_jpeg_entropy(b, len(b), ctypes.byref(info), out.ctypes.data, out.ctypes.data + 2 * info.coef_count)
                times[label].append(time.perf_counter() - t0)
                assert rc == 0, "%s refused file %d" % (label, i)
        if r:
            for label in times:
                rounds[label].append(med(times[label]) * 1e3)
    for label, _L in libs:
        say("  %-10s %.4f ms   (rounds: %s; spread %.4f)" % (label, med(rounds[label]), " ".join("%.4f" % t for t in rounds[label]),
                                                            max(rounds[label]) - min(rounds[label])))
    a, b = med(rounds["this tree"]), med(rounds["other tree"])
    say("  this tree / other tree = %.4f" % (a / b))


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    if args.entropy_against:
        entropy_ab(say)
        log = args.log or os.path.join(ROOT, "profiles", "jpeg_loud_cost.log")
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    from ssd_amd._lib import SsdJpegImage, SsdJpegInfo, lib
    d = tempfile.mkdtemp(prefix="val_like_")
    t0 = time.perf_counter()
    gt = write_folder(d, args.images)
    blobs = [open(os.path.join(d, m["file_name"]), "rb").read() for m in gt["images"]]
    say("%d JPEGs, %.0f KB each, written in %.1f s" % (len(blobs), sum(map(len, blobs)) / 1024 / len(blobs), time.perf_counter() - t0))

    # ---- per image, one core
    import io
    sample = blobs[:min(len(blobs), 208)]
    t_pil = []
    for b in sample:
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        t_pil.append(time.perf_counter() - t0)
    L = lib()
    pin = torch.empty((64 << 20,), dtype=torch.uint8).pin_memory()
    t_ent, refused = [], 0
    for b in sample:
        info = SsdJpegInfo()
        t0 = time.perf_counter()
        rc = L.ssd_jpeg_info_read(b, len(b), ctypes.byref(info))
        if rc == 0:
            rc = L.ssd_jpeg_entropy(b, len(b), ctypes.byref(info), pin.data_ptr(), pin.data_ptr() + 2 * info.coef_count)
        t_ent.append(time.perf_counter() - t0)
        refused += rc != 0
    assert refused == 0
    say("per image, one core:  PIL decode %.2f ms   ssd_jpeg_info_read + ssd_jpeg_entropy %.2f ms   (medians over %d files)"
        % (med(t_pil) * 1e3, med(t_ent) * 1e3, len(sample)))

    # ---- per 32-image batch: the upload and the two launches, by HIP events
    say("device: %s" % torch.cuda.get_device_name(0))
    t_up, t_k, mb = [], [], []
    for k in range(0, len(blobs) - 31, 32):
        part = blobs[k:k + 32]
        infos = (SsdJpegInfo * 32)()
        for j, b in enumerate(part):
            assert L.ssd_jpeg_info_read(b, len(b), ctypes.byref(infos[j])) == 0
        table, totals = (SsdJpegImage * 32)(), (ctypes.c_int64 * 4)()
        assert L.ssd_jpeg_plan(infos, 32, table, totals) == 0
        quant_at = (2 * totals[0] + 15) & ~15
        table_at = (quant_at + 2 * totals[1] + 15) & ~15
        used = table_at + ctypes.sizeof(table)
        for j, b in enumerate(part):
            assert L.ssd_jpeg_entropy(b, len(b), ctypes.byref(infos[j]), pin.data_ptr() + 2 * table[j].coef_offset,
                                      pin.data_ptr() + quant_at + 2 * table[j].quant_offset) == 0
        ctypes.memmove(pin.data_ptr() + table_at, table, ctypes.sizeof(table))
        dev = torch.empty((used,), dtype=torch.uint8, device="cuda:0")
        ws = torch.empty((int(L.ssd_jpeg_workspace_bytes(table, 32)),), dtype=torch.uint8, device="cuda:0")
        flat = torch.empty((int(totals[3]),), dtype=torch.uint8, device="cuda:0")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for rep in range(2):                                    # (the second repetition is the timed one)
            torch.cuda.synchronize()
            ev[0].record()
            dev.copy_(pin[:used], non_blocking=True)
            ev[1].record()
            ssd_amd._lib.check(L.ssd_jpeg_decode(table, dev.data_ptr() + table_at, 32, dev.data_ptr(), dev.data_ptr() + quant_at,
                                                 ws.data_ptr(), flat.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            ev[2].record()
            torch.cuda.synchronize()
        t_up.append(ev[0].elapsed_time(ev[1]))
        t_k.append(ev[1].elapsed_time(ev[2]))
        mb.append(used / 1e6)
        if k == 0:                                              # the frames are PIL's
            host = flat.cpu().numpy()
            for j, b in enumerate(part):
                want = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
                assert np.array_equal(host[table[j].frame_offset:table[j].frame_offset + want.size].reshape(want.shape), want)
    say("per 32-image batch (HIP events, medians over %d batches): upload of %.1f MB %.3f ms = %.1f GB/s; the two launches %.3f ms"
        % (len(t_up), med(mb), med(t_up), med(mb) / med(t_up), med(t_k)))
    say("per image: upload %.3f ms, the two launches %.4f ms" % (med(t_up) / 32, med(t_k) / 32))

    # ---- end to end
    def relay():
        if not args.parent:
            return
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.parent, "--folder", d, "--rounds", str(args.rounds)],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        for line in out.stdout.splitlines():
            if line.startswith("  parent"):
                say(line)
    say("coco_eval.evaluate, files -> the twelve statistics, %d images, read_workers default (%d CPUs visible), max_batch 32:"
        % (len(blobs), os.cpu_count()))
    relay()
    det = ssd_amd.Detector(ssd_amd.synthetic_weights(P, seed=0, logits_bias=-7.5), config=P)
    harness(det, gt, d, ROUTES, args.rounds, say, "this tree")
    relay()
    say("every route's statistics and predictions file equal the default route's in every round")
    say("no ratio was promised in advance, this is what was measured")
    log = args.log or os.path.join(ROOT, "profiles", "jpeg_decode_cost.log")
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if args.tree else main()
