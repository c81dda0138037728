"""The TRAIN input pipeline's cost: ssd_augment at 640x640 for B = 8, 32, 64 in NHWC and NCHW with every flag off and
with every flag on (kernel milliseconds by HIP events, frames already on the device; effective TB/s = (output bytes +
the crop windows' source bytes) / time), then TrainPipeline's images/s over a synthetic COCO-like shard (480x640-ish
JPEGs, 16 decode threads) and the fraction of the wall time the consumer waited on a decode.
usage: python scripts/augment_cost.py [--pipeline-batches N]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import ssd_amd
from ssd_amd import augment, tfrecords
from helpers import example_protos

ap = argparse.ArgumentParser()
ap.add_argument("--pipeline-batches", type=int, default=40)
a = ap.parse_args()

rng = np.random.default_rng(0)
SRC = [(480, 640), (427, 640), (640, 480), (375, 500), (640, 640), (333, 500), (612, 612), (480, 640)]
print("ssd_augment, 640x640 output, frames of COCO-like sizes on the device, crop windows ~0.8 of the frame")
for B in (8, 32, 64):
    shapes = [SRC[i % len(SRC)] for i in range(B)]
    frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for H, W in shapes]
    params = np.zeros(B, augment.PARAMS_DTYPE)
    for b, (H, W) in enumerate(shapes):
        h, w = int(H * 0.9), int(W * 0.9)
        params[b]["crop_y"], params[b]["crop_x"], params[b]["crop_h"], params[b]["crop_w"] = (H - h) // 2, (W - w) // 2, h, w
        params[b]["color_offset"] = (0.05, -0.02, 0.03)
        params[b]["scale_min"], params[b]["scale_range"] = np.float32(0.85), np.float32(1.15) - np.float32(0.85)
        params[b]["philox_key"] = 1234567 + b
    in_bytes = int(sum(int(p["crop_h"]) * int(p["crop_w"]) * 3 for p in params))
    out_bytes = B * 640 * 640 * 3 * 4
    for cf in (False, True):
        for flags in (0, 15):
            params["flags"] = flags
            for _ in range(3):
                ssd_amd.augment_batch(frames, params, (640, 640), channels_first=cf)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ts = []
            out = torch.empty((B, 640, 640, 3), dtype=torch.float32, device="cuda")
            L = ssd_amd.lib()
            import ctypes
            base = min(f.data_ptr() for f in frames)
            params["offset"] = [f.data_ptr() - base for f in frames]
            params["height"] = [f.shape[0] for f in frames]
            params["width"] = [f.shape[1] for f in frames]
            pdev = torch.from_numpy(params.view(np.uint8).copy()).cuda()
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(20):
                ev[0].record()
                ssd_amd._lib.check(L.ssd_augment(ctypes.c_void_p(base), params.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_void_p(pdev.data_ptr()), B, 640, 640, int(cf),
                                                 ctypes.c_void_p(out.data_ptr()), stream))
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
            ms = float(np.median(ts))
            print("  B=%2d %s flags=%s: %.1f us (median of 20; min %.1f) = %.2f TB/s effective (%.0f MB out + %.0f MB in)"
                  % (B, "NCHW" if cf else "NHWC", "all" if flags else "none", ms * 1e3, min(ts) * 1e3,
                     (out_bytes + in_bytes) / (ms * 1e-3) / 1e12, out_bytes / 1e6, in_bytes / 1e6))

# ---- TrainPipeline over a synthetic shard
print("TrainPipeline, batch 32 at 640x640, 16 decode threads, synthetic COCO-like shard")
with tempfile.TemporaryDirectory() as tmp:
    recs = []
    yy, xx = np.mgrid[0:480, 0:640]
    for i in range(256):
        H, W = SRC[i % len(SRC)]
        base = ((np.sin(yy[:H, :W] / (17.0 + i % 7)) + np.cos(xx[:H, :W] / (23.0 + i % 5))) * 60 + 128)
        img = np.clip(base[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8) if H <= 480 and W <= 640 else \
            rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        m = int(rng.integers(1, 12))
        c = rng.uniform(0.0, 0.7, (m, 2))
        boxes = np.concatenate([c, c + rng.uniform(0.05, 0.3, (m, 2))], 1).clip(0, 1)
        recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 80, m)))
    path = os.path.join(tmp, "train-00.tfrecords")
    tfrecords.write_records(path, recs)
    print("  shard: 256 JPEGs, %.1f MB" % (os.path.getsize(path) / 1e6))
    pipe = ssd_amd.TrainPipeline(tmp, {"batch_size": 32, "image_height": 640, "image_width": 640}, seed=0, read_workers=16)
    for _ in range(3):
        images, gt = next(pipe)
    torch.cuda.synchronize()
    pipe.wait_seconds = 0.0
    t0 = time.perf_counter()
    for _ in range(a.pipeline_batches):
        images, gt = next(pipe)
        images.sum()                          # a consumer that touches the batch on its stream
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = a.pipeline_batches * 32
    print("  %d batches: %.0f img/s, consumer waited on decodes %.1f %% of the wall time (%.2f of %.2f s)"
          % (a.pipeline_batches, n / dt, 100 * pipe.wait_seconds / dt, pipe.wait_seconds, dt))
