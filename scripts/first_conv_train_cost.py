"""What training Conv2d_0 costs (include/ssd_hip.h, "the TRAIN first convolution"): with HIP events, at 8 and 32 frames of 640 x 896
(Conv2d_0's output is 320 x 448 x 32), num_classes 80.

    python scripts/first_conv_train_cost.py [--frames 8 32] [--reps 5] [--no-step]

Reports the raw forward, the weight gradient and the batch norm + ReLU6 of Conv2d_0; the backbone alone and one whole backbone + FPN +
head step (forward, loss, backward) with train_first off and on IN THE SAME RUN, each with its peak of
torch.cuda.max_memory_allocated.  Yardsticks for the weight gradient: (bytes of dy + bytes of images) over the time against the
depthwise weight gradient of Conv2d_1 (1.2 TB/s) and the depthwise data gradient (4.7 TB/s) of DESIGN.md 4.13, and its
27 * Cout * rows double FMAs over the time.  There is no speed gate."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd._lib import SsdBnLevel, check, lib                   # noqa: E402
from head_train_cost import timed                                 # noqa: E402


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def first_conv_lines(B, H, W, Cout, reps):
    L, s = lib(), stream()
    g = torch.Generator(device="cuda").manual_seed(1)
    OH, OW = H // 2, W // 2
    images = torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    w = torch.randn((3, 3, 3, Cout), device="cuda", generator=g)
    dy = torch.randn((B, OH, OW, Cout), device="cuda", generator=g)
    y, dw = torch.empty_like(dy), torch.empty_like(w)
    ws = torch.empty(L.ssd_first_conv_train_workspace_bytes(B, H, W, Cout), dtype=torch.uint8, device="cuda")
    t_f = timed(lambda: check(L.ssd_first_conv_train_forward(images.data_ptr(), B, H, W, w.data_ptr(), Cout, y.data_ptr(), s)), reps)
    t_w = timed(lambda: check(L.ssd_first_conv_train_backward(images.data_ptr(), dy.data_ptr(), B, H, W, Cout, dw.data_ptr(), ws.data_ptr(),
                                                              ws.numel(), s)), reps)
    nb = images.numel() + dy.numel() * 4.0
    fma = 27.0 * Cout * B * OH * OW
    print("  Conv2d_0  3 -> %d channels, stride 2, %dx%d  images %.1f MB, output / dy %.1f MB  workspace %.2f MB"
          % (Cout, H, W, images.numel() / 1e6, dy.numel() * 4 / 1e6, ws.numel() / 1e6))
    print("    forward (raw)                         %8.3f ms  %7.1f GB/s" % (t_f, nb / t_f / 1e6))
    print("    weight gradient (partial + final)     %8.3f ms  %7.1f GB/s  %6.2f T double FMA/s (%.2e FMAs)" % (t_w, nb / t_w / 1e6, fma / t_w / 1e9, fma))
    # the batch norm + ReLU6 on Conv2d_0's output
    x = torch.randn((B * OH * OW, Cout), device="cuda", generator=g) * 2
    d2 = torch.randn_like(x)
    yy, dx = torch.empty_like(x), torch.empty_like(x)
    v = [torch.ones(Cout, device="cuda") for _ in range(9)]
    lv = (SsdBnLevel * 1)(SsdBnLevel(x.shape[0], x.data_ptr(), d2.data_ptr(), yy.data_ptr(), *[t.data_ptr() for t in v]))
    bws = torch.empty(max(L.ssd_bn_relu_train_workspace_bytes(lv, 1, Cout), 256), dtype=torch.uint8, device="cuda")
    t_bf = timed(lambda: check(L.ssd_bn_act_train_forward(lv, 1, Cout, 2, 1, 1e-3, 0.007, bws.data_ptr(), bws.numel(), s)), reps)
    lv[0].out = dx.data_ptr()
    t_bb = timed(lambda: check(L.ssd_bn_act_train_backward(lv, 1, Cout, 2, bws.data_ptr(), bws.numel(), s)), reps)
    xb = x.numel() * 4.0
    print("    batch norm + ReLU6 forward  (3 reads + 1 write) %6.3f ms  %7.1f GB/s" % (t_bf, 4 * xb / t_bf / 1e6))
    print("    batch norm + ReLU6 backward (4 reads + 1 write) %6.3f ms  %7.1f GB/s" % (t_bb, 5 * xb / t_bb / 1e6))


def step_lines(B, reps):
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
    W = ssd_amd.synthetic_weights(params, seed=1)
    g = torch.Generator(device="cuda").manual_seed(4)
    images = torch.randint(0, 256, (B, 640, 896, 3), device="cuda", generator=g, dtype=torch.uint8)
    anchors = torch.from_numpy(ssd_amd.AnchorGenerator()(640, 896)).cuda()
    boxes = np.tile(np.array([[[0.2, 0.2, 0.6, 0.7], [0.5, 0.1, 0.9, 0.4]]], np.float32), (B, 1, 1))
    gt = {"boxes": boxes, "labels": np.ones((B, 2), np.int32), "num_boxes": np.full(B, 2, np.int32)}
    fpn = ssd_amd.TrainableFPN(params, W, device="cuda").train()
    head = ssd_amd.TrainableBoxPredictor(params, W, device="cuda").train()
    res = {}
    for train_first in (False, True):
        backbone = ssd_amd.TrainableMobileNet(params, W, device="cuda", train_first=train_first).train()
        modules = (backbone, fpn, head)

        def clear():
            for m in modules:
                for p in m.parameters():
                    p.grad = None

        def backbone_only():
            clear()
            cs = backbone(images)
            torch.autograd.backward(cs, [torch.ones_like(c) for c in cs])

        def step():
            clear()
            eb, cp = head(fpn(backbone(images)))
            out = ssd_amd.differentiable_loss(cp, eb, anchors, gt, {"gamma": 2.0, "alpha": 0.25})
            (out["localization_loss"] + out["classification_loss"]).backward()
        for what, fn in (("the backbone alone, forward + backward", backbone_only), ("one backbone + FPN + head step (forward + loss + backward)", step)):
            clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t = timed(fn, reps)
            res[(what, train_first)] = t
            print("  train_first=%-5s  %-58s %8.2f ms  peak memory %.2f GB" % (train_first, what, t, torch.cuda.max_memory_allocated() / 1e9))
        del backbone
    for what in sorted({k[0] for k in res}):
        print("  train_first on - off: %-58s %+8.2f ms" % (what, res[(what, True)] - res[(what, False)]))


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
            step_lines(B, max(1, a.reps // 2))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
