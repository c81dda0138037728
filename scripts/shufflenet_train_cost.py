"""What one training step of the ShuffleNet backbone costs (include/ssd_hip.h, "the TRAIN ShuffleNet"), with HIP events, at config 4's
size: 8 frames of 640 x 640, depth_multiplier 1.0 (MaxPool's output is 160 x 160 x 24, the Stage2 halves 80 x 80 x 58).

    python scripts/shufflenet_train_cost.py [--frames 8] [--reps 5] [--rounds 5]

1. Per op, the forward and backward time of ONE step of TrainableShuffleNet (train_first=True): every call of train_calls.py is
   bracketed by two events, and the times are added per entry-point family over the step.  The events sit between the launches, so
   a family's time leaves out what torch does between two calls (allocation, autograd bookkeeping) and holds the events' own cost;
   the module total, measured around the whole forward + backward without the brackets, is printed beside the sum.
2. The depthwise data gradient and weight gradient at 80 x 80 (Stage2, stride 1) for C = 56, 58 and 60 in GB/s of the bytes each has
   to move (dx: dy read, dx written; dw: x and dy read): 56 and 60 run the kernels on 16-byte accesses, 58 the same kernels on 8-byte
   accesses.  The three widths alternate inside one run, `--rounds` times; the median and the spread of each are printed.  The entry
   point always computes dw, so "dx" is a DIFFERENCE of two timings (the backward with dx minus the backward without): it carries
   the noise of both and whatever the dx launch overlaps with the dw kernels -- the cost of asking for dx, not that kernel alone."""
import argparse
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import train_calls as calls                          # noqa: E402
from head_train_cost import timed                                 # noqa: E402

PARAMS = {"backbone": "shufflenet", "depth_multiplier": 1.0, "num_classes": 80}
OPS = OrderedDict([("first_conv_forward", "first convolution, forward"), ("first_conv_backward", "first convolution, weight gradient"),
                   ("conv_forward", "1x1 convolution, forward"), ("conv_backward", "1x1 convolution, dw + dx"),
                   ("depthwise_forward", "depthwise, forward"), ("depthwise_backward", "depthwise, dw + dx"),
                   ("bn_forward", "batch norm (+ ReLU), forward"), ("bn_backward", "batch norm (+ ReLU), backward"),
                   ("shuffle", "concat_shuffle_split, forward + backward"), ("concat", "stage concat, forward"),
                   ("split", "stage concat, backward"), ("maxpool_backward", "max pool, backward")])


def step_lines(B, reps):
    W = ssd_amd.synthetic_weights(PARAMS, seed=1)
    m = ssd_amd.TrainableShuffleNet(PARAMS, W, device="cuda", train_first=True).train()
    g = torch.Generator(device="cuda").manual_seed(4)
    images = torch.randint(0, 256, (B, 640, 640, 3), device="cuda", generator=g, dtype=torch.uint8)

    def step():
        for p in m.parameters():
            p.grad = None
        cs = m(images)
        torch.autograd.backward(cs, [torch.ones_like(c) for c in cs])
    torch.cuda.reset_peak_memory_stats()
    total = timed(step, reps)
    print("  the backbone alone (Conv1 trained; forward + backward of 56 convolutions, 56 batch norms, 13 shuffles, 3 concats, 1 max pool)"
          " %8.2f ms  peak memory %.2f GB" % (total, torch.cuda.max_memory_allocated() / 1e9))
    # the same step with every train_calls function bracketed by events
    spans, real = [], {name: getattr(calls, name) for name in OPS}

    def bracket(name):
        def call(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            real[name](*a, **kw)
            e1.record()
            spans.append((name, e0, e1))
        return call
    for name in OPS:
        setattr(calls, name, bracket(name))
    try:
        step()                                                    # (every shape is warm: `timed` has run the step)
        torch.cuda.synchronize()
        del spans[:]
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
    finally:
        for name in OPS:
            setattr(calls, name, real[name])
    ms, n = {name: 0.0 for name in OPS}, {name: 0 for name in OPS}
    for name, e0, e1 in spans:
        ms[name] += e0.elapsed_time(e1) / reps
        n[name] += 1
    for name, label in OPS.items():
        print("    %-42s %4d calls  %8.3f ms" % (label, n[name] // reps, ms[name]))
    print("    %-42s             %8.3f ms  (the step without brackets: %.2f ms)" % ("sum of the bracketed calls", sum(ms.values()), total))
    # the frozen default beside it
    m2 = ssd_amd.TrainableShuffleNet(PARAMS, W, device="cuda").train()

    def step2():
        for p in m2.parameters():
            p.grad = None
        cs = m2(images)
        torch.autograd.backward(cs, [torch.ones_like(c) for c in cs])
    print("  the backbone alone (Conv1 frozen, the default) %8.2f ms" % timed(step2, reps))


def width_lines(B, H, W, widths, reps, rounds):
    g = torch.Generator(device="cuda").manual_seed(1)
    cases = {}
    for C in widths:
        x = torch.randn((B, H, W, C), device="cuda", generator=g)
        dy = torch.randn((B, H, W, C), device="cuda", generator=g)
        w = torch.randn((3, 3, C, 1), device="cuda", generator=g)
        ws = torch.empty(calls.depthwise_workspace_bytes(x, 1, entry="sn_depthwise"), dtype=torch.uint8, device="cuda")
        cases[C] = (x, dy, w, torch.empty_like(x), torch.empty_like(w), torch.empty_like(dy), ws)
    res = {C: {"forward": [], "dx": [], "dw": []} for C in widths}
    for _ in range(rounds):                                       # alternating: 56, 58, 60, 56, 58, 60, ...
        for C in widths:
            x, dy, w, dx, dw, y, ws = cases[C]
            bwd = lambda d: calls.depthwise_backward(x, w, dy, dw, 1, d, workspace=ws, entry="sn_depthwise")
            t_f = timed(lambda: calls.depthwise_forward(x, w, y, 1, entry="sn_depthwise"), reps)
            t_w = timed(lambda: bwd(None), reps)
            t_x = timed(lambda: bwd(dx), reps) - t_w
            nb = 2.0 * x.numel() * 4
            for k, t in (("forward", t_f), ("dx", t_x), ("dw", t_w)):
                res[C][k].append(nb / t / 1e6)
    print("  depthwise stride 1 at %dx%d, %d frames, GB/s of (one tensor in + one out | two in): median [min .. max] of %d alternating rounds"
          % (H, W, B, rounds))
    print("  (dx = backward with dx minus backward without it: a difference of two timings, not the dx kernel alone)")
    med = {}
    for C in widths:
        parts = []
        for k in ("forward", "dx", "dw"):
            v = sorted(res[C][k])
            med[(C, k)] = v[len(v) // 2]
            parts.append("%s %7.1f [%7.1f .. %7.1f]" % (k, v[len(v) // 2], v[0], v[-1]))
        print("    C = %3d (%2d-byte accesses)  %s" % (C, 16 if C % 4 == 0 else 8, "   ".join(parts)))
    if 58 in widths and 56 in widths and 60 in widths:
        for k in ("forward", "dx", "dw"):
            print("    %-7s C = 58 against the mean of 56 and 60: %.2f x the bytes per second"
                  % (k, med[(58, k)] / (0.5 * (med[(56, k)] + med[(60, k)]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shufflenet_train_cost.py needs a GPU: nothing here is measured without one")
    print("device:", torch.cuda.get_device_name(0))
    print("%d frames of 640 x 640, ShuffleNet-v2 depth 1.0" % a.frames)
    step_lines(a.frames, a.reps)
    torch.cuda.empty_cache()
    width_lines(a.frames, 80, 80, (56, 58, 60), 20 * a.reps, a.rounds)


if __name__ == "__main__":
    main()
