"""What one step of ssd_amd.Trainer costs, and ssd_train_norms beside ssd_train_update, with HIP events, in ONE run
on one device:

    python scripts/train_step_cost.py [--frames 8 32] [--steps 6] [--reps 20] [--rounds 5] [--no-step]

  the norms beside the update   both entry points over the table of the whole MobileNet model (191 tensors, 14.3 M elements), every
                                gradient present, alternating; warm-up, `--reps` launches per timing, `--rounds` rounds, the median and
                                the spread, and GB/s over the bytes that must move: 2 arrays read per element for the norms (two
                                launches), 5 read + 4 written for the update.  The expectation "the norms cost at most what the update
                                costs" is a note to confirm or explain, not a gate.
  a whole Trainer step          the reference's config (MobileNet, 80 classes, 640 x 640) at `--frames` images per batch over a synthetic
                                COCO-like shard: `--steps` steps after two of warm-up, HIP events around every step() on the training
                                stream, the median and the spread, images/s over the wall time, the pipeline's wait and the peak memory.
There is no speed gate."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import _lib, ckpt_export, tfrecords, train_calls, train_step   # noqa: E402
from head_train_cost import timed                                 # noqa: E402

PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15, "iou_threshold": 0.6,
          "max_boxes_per_class": 25, "min_dimension": 640}
CONFIG = dict(PARAMS, weight_decay=5e-5, localization_loss_weight=1.0, classification_loss_weight=2.0, gamma=2.0, alpha=0.25,
              num_steps=350000, initial_learning_rate=1e-4, image_height=640, image_width=640)


def norms_lines(reps, rounds):
    W = ssd_amd.synthetic_weights(PARAMS, seed=1)
    names = train_step.trainable_names(PARAMS)
    g = torch.Generator(device="cuda").manual_seed(2)
    P = {n: torch.from_numpy(W[n]).cuda().requires_grad_() for n in names}
    ts = ssd_amd.TrainStep(P, CONFIG, layout="tf", params=PARAMS)
    for p in P.values():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
    T, N = len(names), sum(p.numel() for p in P.values())
    rows = ts.gradient_rows()
    host = torch.from_numpy(rows.view(np.uint8).copy())
    dev = host.cuda()
    sums = torch.empty((T, 2), dtype=torch.float64, device="cuda")
    bad = torch.empty((T, 2), dtype=torch.int64, device="cuda")
    ws = torch.empty(train_calls.train_norms_workspace_bytes(host), dtype=torch.uint8, device="cuda")
    scalars = train_step.step_scalars(ts.config, 1)
    L = ssd_amd.lib()

    def update():
        _lib.check(L.ssd_train_update(host.data_ptr(), dev.data_ptr(), T, ctypes.byref(scalars), torch.cuda.current_stream().cuda_stream))
    runs = {"ssd_train_norms  (2 launches)": (lambda: train_calls.train_norms(host, dev, sums, bad, workspace=ws), 2 * 4.0 * N),
            "ssd_train_update (1 launch)": (update, 9 * 4.0 * N)}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _nb) in runs.items():
            times[k].append(timed(fn, reps))
    print("the norms beside the update: %d tensors, %.2f M elements, %d blocks, workspace %.1f KB; %d rounds of %d launches, alternating"
          % (T, N / 1e6, ts.blocks, ws.numel() / 1e3, rounds, reps))
    med = {}
    for k, (_fn, nb) in runs.items():
        t = sorted(times[k])
        med[k] = t[len(t) // 2]
        print("  %-30s median %7.4f ms (%.4f .. %.4f)  %6.3f TB/s over %.0f MB" % (k, med[k], t[0], t[-1], nb / med[k] / 1e9, nb / 1e6))
    a, b = (med[k] for k in runs)
    print("  norms / update = %.2f" % (a / b))
    assert int(bad.sum()) == 0 and bool(torch.isfinite(sums).all())


def shard(tmp, n=128, seed=0):
    from helpers import example_protos
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        H, W = int(rng.integers(360, 640)), int(rng.integers(360, 640))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        m = int(rng.integers(1, 12))
        c = rng.uniform(0.0, 0.7, (m, 2))
        boxes = np.concatenate([c, c + rng.uniform(0.05, 0.3, (m, 2))], 1).clip(0, 1)
        recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 80, m)))
    os.makedirs(os.path.join(tmp, "train"))
    tfrecords.write_records(os.path.join(tmp, "train", "train-00.tfrecords"), recs)
    W = ssd_amd.synthetic_weights(PARAMS, seed=1)
    return ckpt_export.write_checkpoint(os.path.join(tmp, "pretrained.ckpt"), {k: v for k, v in W.items() if k.startswith("MobilenetV1/")})


def step_lines(tmp, pretrained, B, steps):
    cfg = dict(CONFIG, batch_size=B, model_dir=os.path.join(tmp, "run%d" % B), train_dataset=os.path.join(tmp, "train"),
               val_dataset=os.path.join(tmp, "train"), pretrained_checkpoint=pretrained)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t = ssd_amd.Trainer(cfg, seed=0, read_workers=16)
    t.log_every = 0
    for _ in range(2):
        t.step()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    wait0, t0 = t._pipe.wait_seconds, time.perf_counter()
    for e0, e1 in events:
        e0.record()
        t.step()
        e1.record()
    t.drain()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
    print("a whole Trainer step, %2d frames of 640 x 640: median %8.2f ms (%.2f .. %.2f) on the stream; %d steps in %.2f s wall = %.1f img/s; "
          "pipeline wait %.2f s; peak memory %.2f GB; loss %.4f" % (B, ms[len(ms) // 2], ms[0], ms[-1], steps, wall, steps * B / wall,
                                                                    t._pipe.wait_seconds - wait0, torch.cuda.max_memory_allocated() / 1e9,
                                                                    t.last["loss"]))
    t.close_pipeline()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    norms_lines(a.reps, a.rounds)
    if a.no_step:
        return
    with tempfile.TemporaryDirectory() as tmp:
        pretrained = shard(tmp)
        for B in a.frames:
            step_lines(tmp, pretrained, B, a.steps)


if __name__ == "__main__":
    main()
