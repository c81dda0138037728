"""What train.py's summaries cost, with HIP events, in ONE run on one device:

    python scripts/summary_cost.py [--frames 8] [--steps 6] [--reps 20] [--rounds 5] [--no-step] [--contention-only]

  the histograms beside the update and the norms
        ssd_train_histograms over the table of the whole MobileNet model (191 tensors, 14.3 M elements) with realistic values: the
        variance-scaling weights a Trainer starts from and the gradients of one real step at `--frames` images.  Timed in alternating
        rounds against ssd_train_norms and ssd_train_update on the same table (the update with alpha = 0, so that the variables keep
        their values through the timing), under every value of option "hist_scheme" (0 is the naive form: one LDS atomic per element),
        and against the same histograms and statistics computed tensor by tensor with torch ops (searchsorted + bincount + reductions).
        GB/s over the bytes that must move: 2 arrays read per element.
  a whole Trainer step with and without a due summary
        the reference's config at `--frames` images: alternating rounds of `--steps` steps with save_summary_steps = 1 and = 0, HIP
        events around every step() on the training stream and the wall time per step (the event file is written on the host).
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import _lib, train_calls, train_step                 # noqa: E402
from head_train_cost import timed                                 # noqa: E402
from train_step_cost import CONFIG, shard                         # noqa: E402

UNSET = -2 ** 31
SCHEMES = ((UNSET, "default"), (0, "0: an atomic per element"), (1, "1: one ballot"), (2, "2: 1 round"), (3, "3: 2 rounds"),
           (4, "4: rounds until none pends"))


def contention_lines(reps, rounds):
    """256 tensors of 64 Ki elements, no gradients, under every scheme: a constant (every lane of every wave on ONE LDS address), two
    values drawn at random, and a normal draw (the realistic case).  Many tensors, so that neither stage 2's serial chain over one
    tensor's partials nor the flush of every block into one row of counts hides what the LDS atomics cost."""
    T, each = 256, 64 << 10
    n = T * each
    g = torch.Generator(device="cuda").manual_seed(3)
    cases = {"constant": torch.full((n,), 0.125, device="cuda"),
             "two values": torch.where(torch.rand(n, device="cuda", generator=g) < 0.5, 0.75, -3e-5).float(),
             "normal(0, 0.05)": torch.randn(n, device="cuda", generator=g) * 0.05}
    limits = torch.from_numpy(train_calls.histogram_limits().copy()).cuda()
    counts = torch.empty((T, 2, limits.numel()), dtype=torch.int64, device="cuda")
    stats = torch.empty((T, 2, train_calls.STATS_BYTES), dtype=torch.uint8, device="cuda")
    print("%d tensors of %d Ki elements without gradients (%d MB read), ms per call under each hist_scheme:" % (T, each >> 10, n * 4 >> 20))
    for label, w in cases.items():
        rows = np.zeros(T, train_step.TENSOR_DTYPE)
        rows["w"] = rows["m"] = rows["v"] = rows["ema"] = w.data_ptr() + 4 * each * np.arange(T, dtype=np.uint64)
        rows["count"] = each
        rows["first_block"] = train_step.block_starts(rows["w"], rows["count"])[0]
        host = torch.from_numpy(rows.view(np.uint8).copy())
        dev = host.cuda()
        ws = torch.empty(train_calls.train_histograms_workspace_bytes(host), dtype=torch.uint8, device="cuda")
        med = []
        for scheme, _l in SCHEMES[1:]:
            ssd_amd.set_option("hist_scheme", scheme)
            t = sorted(timed(lambda: train_calls.train_histograms(host, dev, 0.0, limits, counts, stats, workspace=ws), reps) for _ in range(rounds))
            ssd_amd.set_option("hist_scheme", UNSET)
            med.append(t[len(t) // 2])
            assert int(counts.sum()) == n
        print("  %-16s %s   (%d occupied buckets in the first tensor)" % (label, "  ".join("%d: %7.4f" % (s, m) for (s, _l), m in zip(SCHEMES[1:], med)),
                                                      int((counts[0] != 0).sum())))


def torch_histograms(params, decay, wd, limits):
    """The same outputs tensor by tensor with torch ops: what a loop over the variables costs."""
    out = []
    for p, d in zip(params, decay):
        for x in (p.detach().reshape(-1), (p.grad + wd * p.detach() if d else p.grad).reshape(-1)):
            x64 = x.double()
            counts = torch.bincount(torch.searchsorted(limits, x64, right=True), minlength=limits.numel())
            out.append((counts, x64.sum(), (x64 * x64).sum(), x.min(), x.max(), torch.isfinite(x).sum()))
    return out


def kernel_lines(t, reps, rounds):
    ts = t.train_step
    names = ts.names
    P = [ts.parameters[n] for n in names]
    assert all(p.grad is not None for p in P)
    T, N = len(names), sum(p.numel() for p in P)
    rows = ts.gradient_rows()
    host = torch.from_numpy(rows.view(np.uint8).copy())
    dev = host.cuda()
    limits = torch.from_numpy(train_calls.histogram_limits().copy()).cuda()
    NB = limits.numel()
    counts = torch.empty((T, 2, NB), dtype=torch.int64, device="cuda")
    stats = torch.empty((T, 2, train_calls.STATS_BYTES), dtype=torch.uint8, device="cuda")
    sums = torch.empty((T, 2), dtype=torch.float64, device="cuda")
    bad = torch.empty((T, 2), dtype=torch.int64, device="cuda")
    hws = torch.empty(train_calls.train_histograms_workspace_bytes(host), dtype=torch.uint8, device="cuda")
    nws = torch.empty(train_calls.train_norms_workspace_bytes(host), dtype=torch.uint8, device="cuda")
    scalars = train_step.step_scalars(ts.config, 1)
    scalars.alpha = 0.0                                            # the variables keep their values through the timing
    wd = float(np.float32(ts.config["weight_decay"]))
    L = ssd_amd.lib()

    def update():
        _lib.check(L.ssd_train_update(host.data_ptr(), dev.data_ptr(), T, ctypes.byref(scalars), torch.cuda.current_stream().cuda_stream))

    def hist():
        train_calls.train_histograms(host, dev, wd, limits, counts, stats, workspace=hws)
    decay = [int(d) for d in rows["decay"]]
    runs = {"ssd_train_update (1 launch, alpha 0)": (None, update, 9 * 4.0 * N),
            "ssd_train_norms (2 launches)": (None, lambda: train_calls.train_norms(host, dev, sums, bad, workspace=nws), 2 * 4.0 * N)}
    for scheme, label in SCHEMES:
        runs["ssd_train_histograms, hist_scheme %s" % label] = (scheme, hist, 2 * 4.0 * N)
    runs["torch ops, tensor by tensor (%d tensors x 2 planes)" % T] = (None, lambda: torch_histograms(P, decay, wd, limits), 2 * 4.0 * N)
    times = {k: [] for k in runs}
    reference = None
    for _ in range(rounds):
        for k, (scheme, fn, _nb) in runs.items():
            if scheme is not None:
                ssd_amd.set_option("hist_scheme", scheme)
            times[k].append(timed(fn, reps if "torch" not in k else max(reps // 10, 1)))
            if scheme is not None:
                ssd_amd.set_option("hist_scheme", UNSET)
                got = (counts.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes())
                reference = reference or got
                assert got == reference, "scheme %r changed the result" % (scheme,)
    c = counts.cpu().numpy()
    st = stats.cpu().numpy().view(train_calls.STATS_DTYPE)[:, :, 0]
    assert not st["bad"].any() and (c.sum(axis=2) == st["num"]).all() and int(st["num"][:, 0].sum()) == N
    occupied = (c != 0).sum(axis=2)
    print("the histograms beside the update and the norms: %d tensors, %.2f M elements, %d blocks, NB %d, histogram workspace %.1f KB, "
          "counts %.1f MB; %d rounds of %d launches, alternating" % (T, N / 1e6, ts.blocks, NB, hws.numel() / 1e3, counts.numel() * 8 / 1e6,
                                                                     rounds, reps))
    print("  occupied buckets per plane: median %d, max %d (variables), median %d, max %d (gradients)"
          % (np.median(occupied[:, 0]), occupied[:, 0].max(), np.median(occupied[:, 1]), occupied[:, 1].max()))
    med = {}
    for k, (_s, _fn, nb) in runs.items():
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        print("  %-58s median %8.4f ms (%.4f .. %.4f)  %6.3f TB/s over %.0f MB" % (k, med[k], v[0], v[-1], nb / med[k] / 1e9, nb / 1e6))
    keys = list(runs)
    print("  histograms (default) / update = %.2f, / norms = %.2f, torch ops / histograms (default) = %.1f"
          % (med[keys[2]] / med[keys[0]], med[keys[2]] / med[keys[1]], med[keys[-1]] / med[keys[2]]))


def step_lines(t, B, steps, rounds):
    per = {1: [], 0: []}
    wall = {1: [], 0: []}
    for _ in range(rounds):
        for every in (1, 0):
            t.save_summary_steps = every
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
            wall[every].append((time.perf_counter() - t0) / steps * 1e3)
            per[every] += [e0.elapsed_time(e1) for e0, e1 in events]
    for every, label in ((0, "no summary"), (1, "a summary due at every step")):
        ms, w = sorted(per[every]), sorted(wall[every])
        print("a whole Trainer step, %2d frames of 640 x 640, %-28s: median %8.2f ms (%.2f .. %.2f) on the stream; wall %8.2f ms per step "
              "(%.2f .. %.2f)" % (B, label, ms[len(ms) // 2], ms[0], ms[-1], w[len(w) // 2], w[0], w[-1]))
    files = ssd_amd.summaries.event_files(t.model_dir)
    n = sum(len(ssd_amd.summaries.read_events(f)) for f in files)
    print("  event file: %d events, %.1f MB (%.0f KB per event)" % (n, sum(os.path.getsize(f) for f in files) / 1e6,
                                                                   sum(os.path.getsize(f) for f in files) / 1e3 / max(n, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--contention-only", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    if a.contention_only:
        contention_lines(a.reps, a.rounds)
        return
    with tempfile.TemporaryDirectory() as tmp:
        pretrained = shard(tmp)
        cfg = dict(CONFIG, batch_size=a.frames, model_dir=os.path.join(tmp, "run"), train_dataset=os.path.join(tmp, "train"),
                   val_dataset=os.path.join(tmp, "train"), pretrained_checkpoint=pretrained)
        t = ssd_amd.Trainer(cfg, seed=0, read_workers=16)
        t.log_every = 0
        for _ in range(2):
            t.step()                                              # the variables' .grad stay those of the last step
        t.drain()
        torch.cuda.synchronize()
        kernel_lines(t, a.reps, a.rounds)
        contention_lines(a.reps, a.rounds)
        if not a.no_step:
            step_lines(t, a.frames, a.steps, a.rounds)
        t.close_pipeline()


if __name__ == "__main__":
    main()
