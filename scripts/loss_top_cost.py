"""What the per-level top-20 % loss histograms cost, with HIP events, in ONE run on one device:

    python scripts/loss_top_cost.py [--frames 8] [--steps 6] [--reps 20] [--rounds 5] [--no-step] [--log profiles/loss_top_cost.log]

  the call beside the summaries' histograms
        ssd_loss_top_means (2 launches) on the per-anchor planes of one real step of the reference's config (640 x 640, 80 classes) at
        `--frames` images and at four times as many (the same planes tiled: the kernel's cost depends on the values and the sizes
        alone), and ssd_train_histograms over the 10-row table of its [2, K] output (3 launches); beside them, measured in the same
        alternating rounds, section 4.18's three histogram launches over the model's table.  Medians over `--rounds` rounds of `--reps`
        calls.
  a whole Trainer step whose summary is due, with the flag on and off
        alternating rounds of `--steps` steps with save_summary_steps = 1: HIP events around every step() on the training stream and
        the wall time per step.
The one stated expectation: a due step with the flag on costs no more than the existing summary launches add to it; the last line
says whether that held.  There is no speed gate.  Every printed line also goes to `--log`."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
import ssd_amd.ssd as ssd_module                                  # noqa: E402
from ssd_amd import train_calls                                   # noqa: E402
from head_train_cost import timed                                 # noqa: E402
from train_step_cost import CONFIG, shard                         # noqa: E402

_log = None


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def median(values):
    v = sorted(values)
    return v[len(v) // 2], v[0], v[-1]


def kernel_lines(t, planes, reps, rounds):
    """planes: (cls_losses, loc_losses) [B,N] of a real step.  -> the medians in ms: {label: value}."""
    ts = t.train_step
    levels = t.anchors_per_level
    counts = train_calls.loss_top_counts(levels)
    K = sum(counts)
    rows = ts.gradient_rows()
    host = torch.from_numpy(rows.view(np.uint8).copy())
    dev = host.cuda()
    limits = torch.from_numpy(train_calls.histogram_limits().copy()).cuda()
    T = len(ts.names)
    mcounts = torch.empty((T, 2, limits.numel()), dtype=torch.int64, device="cuda")
    mstats = torch.empty((T, 2, train_calls.STATS_BYTES), dtype=torch.uint8, device="cuda")
    hws = torch.empty(train_calls.train_histograms_workspace_bytes(host), dtype=torch.uint8, device="cuda")
    wd = float(np.float32(ts.config["weight_decay"]))
    t._loss_top_histograms(*planes)                               # the Trainer's own table, limits and buffers
    top = t._loss_top
    runs = {"ssd_train_histograms over the model's table (4.18, 3 launches)":
            lambda: train_calls.train_histograms(host, dev, wd, limits, mcounts, mstats, workspace=hws)}
    B0 = planes[0].shape[0]
    for mult in (1, 4):
        cls, loc = (p.repeat(mult, 1).contiguous() for p in planes)
        ws = torch.empty(train_calls.loss_top_workspace_bytes(B0 * mult, levels), dtype=torch.uint8, device="cuda")
        means = torch.empty((2, K), dtype=torch.float32, device="cuda")
        runs["ssd_loss_top_means, B = %2d (2 launches)" % (B0 * mult)] = \
            (lambda cls=cls, loc=loc, means=means, ws=ws: train_calls.loss_top_means(cls, loc, levels, means, workspace=ws))
    runs["ssd_train_histograms over the 10 rows of [2, K] (3 launches)"] = \
        lambda: train_calls.train_histograms(top["host"], top["dev"], 0.0, top["limits"], top["counts"], top["stats"], workspace=hws)
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn, reps))
    nz = [float((p != 0).float().mean()) for p in planes]
    say("the call beside the summaries' histograms: levels %s, k %s, K %d; planes of a real step at B = %d (non-zero: classification "
        "%.1f %%, localisation %.2f %%); %d rounds of %d calls, alternating" % (list(levels), list(counts), K, B0, 100 * nz[0], 100 * nz[1],
                                                                                 rounds, reps))
    med = {}
    for k in runs:
        med[k], lo, hi = median(times[k])
        say("  %-68s median %8.4f ms (%.4f .. %.4f)" % (k, med[k], lo, hi))
    return med


def step_lines(t, B, steps, rounds):
    per, wall = {True: [], False: []}, {True: [], False: []}
    t.save_summary_steps = 1
    for _ in range(rounds):
        for flag in (True, False):
            t.loss_histograms = flag
            t.drain()
            torch.cuda.synchronize()
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            t0 = time.perf_counter()
            for e0, e1 in events:
                e0.record()
                t.step()
                e1.record()
            t.drain()
            torch.cuda.synchronize()
            wall[flag].append((time.perf_counter() - t0) / steps * 1e3)
            per[flag] += [e0.elapsed_time(e1) for e0, e1 in events]
    out = {}
    for flag, label in ((False, "flag off"), (True, "flag on")):
        (m, lo, hi), (w, wlo, whi) = median(per[flag]), median(wall[flag])
        out[flag] = (m, w)
        say("a whole Trainer step with a summary due, %2d frames of 640 x 640, %-8s: median %8.2f ms (%.2f .. %.2f) on the stream; wall %8.2f "
            "ms per step (%.2f .. %.2f)" % (B, label, m, lo, hi, w, wlo, whi))
    return out


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "loss_top_cost.log"))
    a = ap.parse_args()
    _log = open(a.log, "w")
    say("device: %s" % torch.cuda.get_device_name(0))
    kept = {}
    inner = ssd_module.differentiable_loss

    def spy(*args, **kwargs):                                     # the per-anchor planes of the steps below
        out = inner(*args, **kwargs)
        if "cls_losses" in out:
            kept["planes"] = (out["cls_losses"].clone(), out["loc_losses"].clone())
        return out
    with tempfile.TemporaryDirectory() as tmp:
        pretrained = shard(tmp)
        cfg = dict(CONFIG, batch_size=a.frames, model_dir=os.path.join(tmp, "run"), train_dataset=os.path.join(tmp, "train"),
                   val_dataset=os.path.join(tmp, "train"), pretrained_checkpoint=pretrained)
        t = ssd_amd.Trainer(cfg, seed=0, read_workers=16)
        t.log_every = 0
        t.save_summary_steps, t.loss_histograms = 1, True
        ssd_module.differentiable_loss = spy
        for _ in range(2):
            t.step()                                              # the variables' .grad stay those of the last step
        ssd_module.differentiable_loss = inner
        t.drain()
        torch.cuda.synchronize()
        med = kernel_lines(t, kept["planes"], a.reps, a.rounds)
        keys = list(med)
        added = med[keys[1]] + med[keys[3]]
        say("  the flag's launches at B = %d: %.4f ms = %.2f x the model's histogram launches (%.4f ms)"
            % (a.frames, added, added / med[keys[0]], med[keys[0]]))
        if not a.no_step:
            steps = step_lines(t, a.frames, a.steps, a.rounds)
            say("  on the stream the flag adds %.2f ms to a due step; the existing summary launches cost %.2f ms there"
                % (steps[True][0] - steps[False][0], med[keys[0]]))
        say("expectation (the flag costs a due step no more than the existing summary launches add): %s"
            % ("held" if added <= med[keys[0]] else "did NOT hold"))
        t.close_pipeline()
    _log.close()


if __name__ == "__main__":
    main()
