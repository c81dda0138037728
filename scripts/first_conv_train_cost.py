"""What training Conv2d_0 costs (include/ssd_hip.h, "the TRAIN first convolution"): with HIP events, at 8 and 32 frames of 640 x 896
(Conv2d_0's output is 320 x 448 x 32), num_classes 80.

    python scripts/first_conv_train_cost.py [--frames 8 32] [--reps 5] [--no-step]

Reports the raw forward, the weight gradient and the batch norm + ReLU6 of Conv2d_0; the backbone alone and one whole backbone + FPN +
head step (forward, loss, backward) with train_first off and on IN THE SAME RUN, each with its peak of
torch.cuda.max_memory_allocated.  Yardsticks for the weight gradient: (bytes of dy + bytes of images) over the time against the
depthwise weight gradient of Conv2d_1 (1.2 TB/s) and the depthwise data gradient (4.7 TB/s) of DESIGN.md 4.13, and its
27 * Cout * rows double FMAs over the time.  There is no speed gate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    for B in a.frames:
        print("%d frames of 640 x 896" % B)
        first_conv_lines(B, 640, 896, 32, a.reps)
        torch.cuda.empty_cache()
        if not a.no_step:
            step_lines(B, max(1, a.reps // 2), train_first=(False, True))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
