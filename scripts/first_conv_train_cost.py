"""What training Conv2d_0 costs (include/ssd_hip.h, "the TRAIN first convolution"): with HIP events, at 8 and 32 frames of 640 x 896
(Conv2d_0's output is 320 x 448 x 32), num_classes 80.

    python scripts/first_conv_train_cost.py [--frames 8 32] [--reps 5] [--no-step] [--float]

Reports the raw forward, the weight gradient and the batch norm + ReLU6 of Conv2d_0; the backbone alone and one whole backbone + FPN +
head step (forward, loss, backward) with train_first off and on IN THE SAME RUN, each with its peak of
torch.cuda.max_memory_allocated.  Yardsticks for the weight gradient: (bytes of dy + bytes of images) over the time against the
depthwise weight gradient of Conv2d_1 (1.2 TB/s) and the depthwise data gradient (4.7 TB/s) of DESIGN.md 4.13, and its
27 * Cout * rows double FMAs over the time.  There is no speed gate.
--float: the calls from float32 frames ("the TRAIN first convolution from float frames") BESIDE the uint8 calls in the
same run on the same device -- forward and weight gradient alternating, warm-up, `--reps` launches per timing, five rounds, the median
and the spread, ms and TB/s over the bytes that must move (frames + output / dy) -- and the backbone alone (train_first=True, forward +
backward) on uint8 against float32 frames with its peak memory."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import train_calls as calls                          # noqa: E402
from head_train_cost import timed                                 # noqa: E402
from backbone_train_cost import bn_lines, step_lines              # noqa: E402


def first_conv_lines(B, H, W, Cout, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    OH, OW = H // 2, W // 2
    images = torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    w = torch.randn((3, 3, 3, Cout), device="cuda", generator=g)
    dy = torch.randn((B, OH, OW, Cout), device="cuda", generator=g)
    y, dw = torch.empty_like(dy), torch.empty_like(w)
    ws = torch.empty(calls.first_conv_workspace_bytes(images, Cout), dtype=torch.uint8, device="cuda")
    t_f = timed(lambda: calls.first_conv_forward(images, w, y), reps)
    t_w = timed(lambda: calls.first_conv_backward(images, dy, dw, workspace=ws), reps)
    nb = images.numel() + dy.numel() * 4.0
    fma = 27.0 * Cout * B * OH * OW
    print("  Conv2d_0  3 -> %d channels, stride 2, %dx%d  images %.1f MB, output / dy %.1f MB  workspace %.2f MB"
          % (Cout, H, W, images.numel() / 1e6, dy.numel() * 4 / 1e6, ws.numel() / 1e6))
    print("    forward (raw)                         %8.3f ms  %7.1f GB/s" % (t_f, nb / t_f / 1e6))
    print("    weight gradient (partial + final)     %8.3f ms  %7.1f GB/s  %6.2f T double FMA/s (%.2e FMAs)" % (t_w, nb / t_w / 1e6, fma / t_w / 1e9, fma))
    bn_lines(B, OH, OW, Cout, reps, inline=True)                     # on Conv2d_0's output


def float_lines(B, H, W, Cout, reps, rounds=5):
    """The float calls beside the uint8 calls on the same frames (x = u * (1 / 255): both compute the same bits), alternating."""
    g = torch.Generator(device="cuda").manual_seed(1)
    OH, OW = H // 2, W // 2
    u8 = torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    x = u8.float() * float(np.float32(1.0 / 255.0))
    w = torch.randn((3, 3, 3, Cout), device="cuda", generator=g)
    dy = torch.randn((B, OH, OW, Cout), device="cuda", generator=g)
    y, dw = torch.empty_like(dy), torch.empty_like(w)
    ws = torch.empty(calls.first_conv_f32_workspace_bytes(x, Cout), dtype=torch.uint8, device="cuda")
    runs = {"uint8   forward": (lambda: calls.first_conv_forward(u8, w, y), u8.numel()),
            "float32 forward": (lambda: calls.first_conv_f32_forward(x, w, y), x.numel() * 4),
            "uint8   weight gradient": (lambda: calls.first_conv_backward(u8, dy, dw, workspace=ws), u8.numel()),
            "float32 weight gradient": (lambda: calls.first_conv_f32_backward(x, dy, dw, workspace=ws), x.numel() * 4)}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _nb) in runs.items():
            times[k].append(timed(fn, reps))
    print("  Conv2d_0  3 -> %d channels, %dx%d: frames %.1f MB uint8 / %.1f MB float32, output / dy %.1f MB; %d rounds of %d launches, alternating"
          % (Cout, H, W, u8.numel() / 1e6, x.numel() * 4 / 1e6, dy.numel() * 4 / 1e6, rounds, reps))
    for k, (_fn, nb) in runs.items():
        t = sorted(times[k])
        med = t[len(t) // 2]
        print("    %-24s median %7.3f ms (%.3f .. %.3f)  %6.3f TB/s over %.0f MB" % (k, med, t[0], t[-1], (nb + dy.numel() * 4.0) / med / 1e9,
                                                                                      (nb + dy.numel() * 4.0) / 1e6))


def float_step_lines(B, reps, rounds=5):
    """The backbone alone with Conv2d_0 trained, forward + backward, on uint8 and on float32 frames, alternating."""
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
    W = ssd_amd.synthetic_weights(params, seed=1)
    g = torch.Generator(device="cuda").manual_seed(4)
    u8 = torch.randint(0, 256, (B, 640, 896, 3), device="cuda", generator=g, dtype=torch.uint8)
    frames = {"uint8": u8, "float32": u8.float() * float(np.float32(1.0 / 255.0))}
    backbone = ssd_amd.TrainableMobileNet(params, W, device="cuda", train_first=True).train()

    def run(images):
        for p in backbone.parameters():
            p.grad = None
        cs = backbone(images)
        torch.autograd.backward(cs, [torch.ones_like(c) for c in cs])
    times, peak = {k: [] for k in frames}, {}
    for _ in range(rounds):
        for k, images in frames.items():
            for p in backbone.parameters():
                p.grad = None
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            times[k].append(timed(lambda: run(images), reps))
            peak[k] = torch.cuda.max_memory_allocated() / 1e9
    for k in frames:
        t = sorted(times[k])
        print("  the backbone alone, train_first=True, %-7s frames (%6.1f MB): median %8.2f ms (%.2f .. %.2f)  peak memory %.2f GB"
              % (k, frames[k].numel() * frames[k].element_size() / 1e6, t[len(t) // 2], t[0], t[-1], peak[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--float", dest="float_mode", action="store_true", help="the float32-frame calls beside the uint8 calls")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    for B in a.frames:
        print("%d frames of 640 x 896" % B)
        if a.float_mode:
            float_lines(B, 640, 896, 32, a.reps)
            torch.cuda.empty_cache()
            if not a.no_step:
                float_step_lines(B, max(1, a.reps // 2))
            torch.cuda.empty_cache()
            continue
        first_conv_lines(B, 640, 896, 32, a.reps)
        torch.cuda.empty_cache()
        if not a.no_step:
            step_lines(B, max(1, a.reps // 2), train_first=(False, True))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
