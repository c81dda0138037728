"""What the TRAIN step's gradient exchange costs on ONE device, with HIP events, in ONE run:

    python scripts/grad_exchange_cost.py [--frames 8] [--steps 6] [--reps 20] [--rounds 5] [--no-step]

  pack and reduce beside the update   ssd_train_grad_pack and ssd_train_grad_reduce at G = 1, 2, 4, 8 over MobileNet's real table (the
                                      191 trainable tensors as rows of kind 0, the moving statistics as rows of kind 1), and
                                      ssd_train_update over the same parameters, alternating; warm-up, `--reps` launches per timing,
                                      `--rounds` rounds, the median and the spread, and TB/s over the bytes that must move: the
                                      tensors read and one slice written for pack, G slices read and the tensors written for reduce.
  a Trainer step with a world-1 group against the plain step   the reference's config at `--frames` images over a synthetic COCO-like
                                      shard, both Trainers in this process, `--rounds` rounds of `--steps` steps each, alternating,
                                      HIP events around every step().  The group is RCCL's with one rank: pack in place, the
                                      all-gather of one slice onto itself, reduce.
What cannot be measured on a box with one GPU: the all-gather between distinct GPUs.  There is no speed gate."""
import argparse
import ctypes
import os
import socket
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import _lib, train_calls, train_step                 # noqa: E402
from head_train_cost import timed                                 # noqa: E402
from train_step_cost import CONFIG, PARAMS, shard                 # noqa: E402

RANKS = (1, 2, 4, 8)


def kernel_lines(reps, rounds):
    W = ssd_amd.synthetic_weights(PARAMS, seed=1)
    names = train_step.trainable_names(PARAMS)
    stats = [n for n in ssd_amd.variable_shapes(PARAMS) if n not in set(names)]
    g = torch.Generator(device="cuda").manual_seed(2)
    P = {n: torch.from_numpy(W[n]).cuda().requires_grad_() for n in names}
    ts = ssd_amd.TrainStep(P, CONFIG, layout="tf", params=PARAMS)
    for p in P.values():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
    S = [torch.from_numpy(W[n]).cuda() for n in stats]
    tensors = [p.grad for p in P.values()] + S
    T, N = len(tensors), sum(t.numel() for t in tensors)
    rows = np.zeros(T, train_calls.REDUCE_ROW_DTYPE)
    rows["count"] = [t.numel() for t in tensors]
    rows["kind"] = [0] * len(P) + [1] * len(S)
    rows["data"] = [t.data_ptr() for t in tensors]
    rows["offset"], slice_floats = train_calls.bucket_layout(rows["count"])
    host = torch.from_numpy(rows.view(np.uint8).copy())
    dev = host.cuda()
    gathered = torch.empty((max(RANKS), slice_floats), dtype=torch.float32, device="cuda")
    header = torch.tensor([37.0, 0.5, 1.5], device="cuda")
    for r in range(max(RANKS)):
        train_calls.train_grad_pack(host, dev, header, gathered[r])
    losses = torch.empty(2, dtype=torch.float32, device="cuda")
    weights = torch.empty(max(RANKS), dtype=torch.float32, device="cuda")
    uhost = torch.from_numpy(ts.gradient_rows().view(np.uint8))
    udev = uhost.cuda()
    scalars = train_step.step_scalars(ts.config, 1)
    L = ssd_amd.lib()

    def update():
        _lib.check(L.ssd_train_update(uhost.data_ptr(), udev.data_ptr(), len(P), ctypes.byref(scalars), torch.cuda.current_stream().cuda_stream))
    # reduce at G ranks averages G equal slices: the gradients keep their size (c_r = 1 / G each), so the update stays finite
    runs = {"ssd_train_grad_pack": (lambda: train_calls.train_grad_pack(host, dev, header, gathered[0]), 4.0 * (N + slice_floats))}
    for G in RANKS:
        runs["ssd_train_grad_reduce G = %d" % G] = (lambda G=G: train_calls.train_grad_reduce(host, dev, gathered[:G], losses, weights[:G]),
                                                    4.0 * (G * slice_floats + N))
    runs["ssd_train_update"] = (update, 9 * 4.0 * sum(p.numel() for p in P.values()))
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _nb) in runs.items():
            times[k].append(timed(fn, reps))
    print("pack and reduce beside the update: %d rows (%d gradients, %d statistics), %.2f M elements, slice %.1f MB; %d rounds of %d launches, "
          "alternating" % (T, len(P), len(S), N / 1e6, 4 * slice_floats / 1e6, rounds, reps))
    med = {}
    for k, (_fn, nb) in runs.items():
        t = sorted(times[k])
        med[k] = t[len(t) // 2]
        print("  %-30s median %7.4f ms (%.4f .. %.4f)  %6.3f TB/s over %.0f MB" % (k, med[k], t[0], t[-1], nb / med[k] / 1e9, nb / 1e6))
    print("  pack + reduce at G = 8: %.4f ms = %.2f x the update" % (med["ssd_train_grad_pack"] + med["ssd_train_grad_reduce G = 8"],
                                                                  (med["ssd_train_grad_pack"] + med["ssd_train_grad_reduce G = 8"]) / med["ssd_train_update"]))
    assert bool(torch.isfinite(losses).all())


def step_lines(tmp, pretrained, B, steps, rounds):
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda", 0))
    cfg = dict(CONFIG, batch_size=B, train_dataset=os.path.join(tmp, "train"), val_dataset=os.path.join(tmp, "train"),
               pretrained_checkpoint=pretrained)
    trainers = {"plain": ssd_amd.Trainer(dict(cfg, model_dir=os.path.join(tmp, "plain")), seed=0, read_workers=16),
                "world-1 group": ssd_amd.Trainer(dict(cfg, model_dir=os.path.join(tmp, "group")), seed=0, read_workers=16,
                                                 group=dist.group.WORLD)}
    ms = {k: [] for k in trainers}
    for t in trainers.values():
        t.log_every = 0
        for _ in range(2):
            t.step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, t in trainers.items():
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for e0, e1 in events:
                e0.record()
                t.step()
                e1.record()
            t.drain()
            torch.cuda.synchronize()
            ms[k] += [e0.elapsed_time(e1) for e0, e1 in events]
    print("a Trainer step, %d frames of 640 x 640, %d rounds of %d steps, alternating:" % (B, rounds, steps))
    med = {}
    for k, v in ms.items():
        v = sorted(v)
        med[k] = v[len(v) // 2]
        print("  %-14s median %8.2f ms (%.2f .. %.2f) on the stream; loss %.4f" % (k, med[k], v[0], v[-1], trainers[k].last["loss"]))
    print("  world-1 group / plain = %.4f (+%.2f ms)" % (med["world-1 group"] / med["plain"], med["world-1 group"] - med["plain"]))
    assert trainers["plain"].last["loss"] == trainers["world-1 group"].last["loss"]       # the exchange at G = 1 is the identity
    for t in trainers.values():
        t.close_pipeline()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    kernel_lines(a.reps, a.rounds)
    if a.no_step:
        return
    with tempfile.TemporaryDirectory() as tmp:
        step_lines(tmp, shard(tmp), a.frames, a.steps, a.rounds)


if __name__ == "__main__":
    main()
