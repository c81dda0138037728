"""The TRAIN update's cost: one ssd_train_update over MobileNet's trainable set (191 tensors, 14 287 672 floats; w, g, m, v, ema
read and w, m, v, ema written = 36 bytes per parameter, 514 MB) beside the same update written with torch._foreach_* ops on the
same tensors -- the baseline, since nothing else in the project can run this step.  Milliseconds by HIP events, bytes per
second, and the share of the 6.3 TB/s a float4 copy reaches on this part.
usage: python scripts/train_update_cost.py [--calls N]   (under `rocprofv3 --kernel-trace --stats --` for the kernel itself)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ssd_amd
from ssd_amd import train_step, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
a = ap.parse_args()
assert a.calls >= 20
COPY_RATE = 6.3e12

PARAMS = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
CFG = {"initial_learning_rate": 1e-4, "num_steps": 350000, "weight_decay": 5e-5}
W = ssd_amd.synthetic_weights(PARAMS, seed=0)
names = train_step.trainable_names(PARAMS)
rng = np.random.default_rng(0)
P = {n: torch.from_numpy(W[n]).cuda().requires_grad_(True) for n in names}
for n in names:
    P[n].grad = torch.from_numpy(rng.normal(0, 1e-2, W[n].shape).astype(np.float32)).cuda()
ts = ssd_amd.TrainStep(P, CFG, layout="tf", params=PARAMS)
count = sum(p.numel() for p in P.values())
nbytes = 36 * count
print("MobileNet trainable set: %d tensors, %d floats, %d launch blocks, %.0f MB moved per update" % (len(names), count, ts.blocks, nbytes / 1e6))


def timed(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return np.array([s.elapsed_time(e) for s, e in ev])


def report(what, ms):
    med = float(np.median(ms))
    print("  %-44s %.4f ms (median of %d; min %.4f) = %.2f TB/s = %.2f of the 6.3 TB/s copy rate"
          % (what, med, len(ms), ms.min(), nbytes / med / 1e9, nbytes / (med * 1e-3) / COPY_RATE))
    return med


step_ms = report("TrainStep.step() (table upload + launch)", timed(ts.step, a.calls))
# the bare launch: the table of the last step() stays valid (the gradients are not reallocated here)
table_host, table_dev = ts._ring.last()
sc = train_step.step_scalars(CFG, ts.global_step + 1)
L = ssd_amd.lib()
stream = torch.cuda.current_stream().cuda_stream


def bare():
    _lib.check(L.ssd_train_update(table_host.data_ptr(), table_dev.data_ptr(), len(names), ctypes.byref(sc), stream))


bare_ms = report("ssd_train_update alone", timed(bare, a.calls))

ws = [P[n].detach() for n in names]
gs = [P[n].grad for n in names]
ms_, vs, es = ([ts.slots(n)[0] for n in names], [ts.slots(n)[1] for n in names], [ts.ema(n) for n in names])
dec = [i for i, n in enumerate(names) if train_step.decays(n)]
s = [float(np.float32(x)) for x in (sc.alpha, sc.one_minus_beta1, sc.one_minus_beta2, sc.epsilon, sc.weight_decay, sc.one_minus_decay)]


def foreach():
    g = list(gs)
    for i, x in zip(dec, torch._foreach_add([gs[i] for i in dec], [ws[i] for i in dec], alpha=s[4])):
        g[i] = x
    d = torch._foreach_sub(g, ms_)
    torch._foreach_mul_(d, s[1])
    torch._foreach_add_(ms_, d)
    d = torch._foreach_mul(g, g)
    torch._foreach_sub_(d, vs)
    torch._foreach_mul_(d, s[2])
    torch._foreach_add_(vs, d)
    den = torch._foreach_sqrt(vs)
    torch._foreach_add_(den, s[3])
    num = torch._foreach_mul(ms_, s[0])
    torch._foreach_div_(num, den)
    torch._foreach_sub_(ws, num)
    d = torch._foreach_sub(es, ws)
    torch._foreach_mul_(d, s[5])
    torch._foreach_sub_(es, d)


fe_ms = report("torch._foreach_* ops, same tensors", timed(foreach, a.calls))
print("  ratio foreach / ssd_train_update: %.1f (against step(): %.1f)" % (fe_ms / bare_ms, fe_ms / step_ms))
print("  nonfinite w after all calls: %d" % sum(int((~torch.isfinite(w)).sum().item()) for w in ws))
