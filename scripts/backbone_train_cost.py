"""What one training step of the MobileNet backbone costs (include/ssd_hip.h, "the TRAIN backbone"): per entry point, with HIP
events, at 8 and 32 frames of 640 x 896 (Conv2d_0's output is 320 x 448 x 32), num_classes 80.

    python scripts/backbone_train_cost.py [--frames 8 32] [--reps 5] [--no-step]

Reports the depthwise forward, data gradient and weight gradient at Conv2d_1 (32 channels, stride 1, 320 x 448), Conv2d_2 (64
channels, stride 2, 320 x 448) and Conv2d_7 (512 channels, stride 1, 40 x 56) in GB/s of the bytes each has to move (forward and
data gradient: one tensor read, one written; weight gradient: both tensors read) -- the yardstick is the inference depthwise
kernel's own rate, 3.7 TB/s at stride 1 and 4.7 TB/s at stride 2 (profiles/r02_depthwise_probe.log) --, the 1x1 data gradient at
512 -> 512 (40 x 56) and 1024 -> 1024 (20 x 28) against the 157.3 TFLOP/s exact-fp32 MFMA peak (yardstick: the 1x1 forward at 0.33
of it), the batch norm with ReLU6 in GB/s, the FPN with and without the bridge to c3, c4, c5, and one whole
backbone + FPN + head step (forward, loss, backward) with its peak memory."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import train_calls as calls                          # noqa: E402
from head_train_cost import PEAK, timed                           # noqa: E402
from fpn_train_cost import C_SIZES, C_WIDTHS                      # noqa: E402


def depthwise_lines(name, B, H, W, C, stride, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    OH, OW = -(-H // stride), -(-W // stride)
    x = torch.randn((B, H, W, C), device="cuda", generator=g)
    dy = torch.randn((B, OH, OW, C), device="cuda", generator=g)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    w = torch.randn((3, 3, C, 1), device="cuda", generator=g)
    dw = torch.empty_like(w)
    ws = torch.empty(calls.depthwise_workspace_bytes(x, stride), dtype=torch.uint8, device="cuda")
    bwd = lambda d: calls.depthwise_backward(x, w, dy, dw, stride, d, workspace=ws)
    t_f = timed(lambda: calls.depthwise_forward(x, w, y, stride), reps)
    t_w = timed(lambda: bwd(None), reps)
    t_x = timed(lambda: bwd(dx), reps) - t_w
    nb = (x.numel() + dy.numel()) * 4.0
    gbs = lambda t: nb / t / 1e6
    print("  %-9s depthwise s%d %4d channels at %dx%d  %.1f MB in + out  workspace %.1f MB" % (name, stride, C, H, W, nb / 1e6, ws.numel() / 1e6))
    print("    forward                               %8.3f ms  %7.1f GB/s" % (t_f, gbs(t_f)))
    print("    data gradient                         %8.3f ms  %7.1f GB/s  (backward with dx minus the weight gradient)" % (t_x, gbs(t_x)))
    print("    weight gradient (partial + final)     %8.3f ms  %7.1f GB/s" % (t_w, gbs(t_w)))


def pointwise_lines(B, H, W, Cin, Cout, reps):
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((B, H, W, Cin), device="cuda", generator=g)
    dy = torch.randn((B, H, W, Cout), device="cuda", generator=g)
    dx = torch.empty_like(x)
    w = torch.randn((1, 1, Cin, Cout), device="cuda", generator=g) * 0.05
    dw = torch.empty_like(w)
    ws = torch.empty(calls.conv_workspace_bytes([x], B, Cin, Cout, 1, entry="pointwise"), dtype=torch.uint8, device="cuda")
    call = lambda dxs: calls.conv_backward([x], w, [dy], dw, dxs=dxs, workspace=ws, entry="pointwise")
    t_w = timed(lambda: call(None), reps)
    t_x = timed(lambda: call([dx]), reps) - t_w
    fl = 2.0 * Cin * Cout * B * H * W
    tf = lambda t: fl / t / 1e9
    print("  1x1 %4d -> %4d at %dx%d  workspace %.1f MB" % (Cin, Cout, H, W, ws.numel() / 1e6))
    print("    weight gradient (wgrad + reduce)      %8.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_w, tf(t_w), 100 * tf(t_w) / PEAK))
    print("    data gradient (permutes + pack + igemm) %6.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_x, tf(t_x), 100 * tf(t_x) / PEAK))


def bn_lines(B, H, W, C, reps, inline=False):
    """inline: two lines under another layer's heading, each naming the batch norm, instead of a heading of its own"""
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((B * H * W, C), device="cuda", generator=g) * 2
    dy = torch.randn_like(x)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta, mm, mv, mean, var, invstd, dgamma, dbeta = [[torch.ones(C, device="cuda")] for _ in range(9)]
    ws = torch.empty(max(calls.bn_workspace_bytes([x], C), 256), dtype=torch.uint8, device="cuda")
    t_f = timed(lambda: calls.bn_forward([x], [y], gamma, beta, True, 1e-3, 0.007, mm, mv, mean, var, invstd, act="relu6", workspace=ws), reps)
    t_b = timed(lambda: calls.bn_backward([x], [dy], [dx], gamma, beta, mean, invstd, dgamma, dbeta, act="relu6", workspace=ws), reps)
    nb = x.numel() * 4.0
    if inline:
        fmt = "    batch norm + ReLU6 %s %6.3f ms  %7.1f GB/s"
    else:
        print("  batch norm + ReLU6, %d channels at %dx%d (%.1f MB)" % (C, H, W, nb / 1e6))
        fmt = "    %s          %8.3f ms  %7.1f GB/s"
    print(fmt % ("forward  (3 reads + 1 write)", t_f, 4 * nb / t_f / 1e6))
    print(fmt % ("backward (4 reads + 1 write)", t_b, 5 * nb / t_b / 1e6))


def step_lines(B, reps, train_first=None):
    """The backbone alone and one whole step.  train_first None: the default backbone (Conv2d_0 frozen), after the FPN alone with and
    without the bridge; a tuple of train_first values: those backbones IN THE SAME RUN under one FPN and head, then on minus off."""
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
    W = ssd_amd.synthetic_weights(params, seed=1)
    fpn = ssd_amd.TrainableFPN(params, W, device="cuda").train()
    head = ssd_amd.TrainableBoxPredictor(params, W, device="cuda").train()
    g = torch.Generator(device="cuda").manual_seed(4)
    images = torch.randint(0, 256, (B, 640, 896, 3), device="cuda", generator=g, dtype=torch.uint8)
    anchors = torch.from_numpy(ssd_amd.AnchorGenerator()(640, 896)).cuda()
    boxes = np.tile(np.array([[[0.2, 0.2, 0.6, 0.7], [0.5, 0.1, 0.9, 0.4]]], np.float32), (B, 1, 1))
    gt = {"boxes": boxes, "labels": np.ones((B, 2), np.int32), "num_boxes": np.full(B, 2, np.int32)}
    BACKBONE, STEP = "the backbone alone, forward + backward", "one backbone + FPN + head step (forward + loss + backward)"

    def clear(*more):
        for m in (fpn, head) + more:
            for p in m.parameters():
                p.grad = None

    def timed_line(label, fn):
        """One line: label, time, peak memory.  -> ms"""
        clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t = timed(fn, reps)
        print("%s %8.2f ms  peak memory %.2f GB" % (label, t, torch.cuda.max_memory_allocated() / 1e9))
        return t

    def fpn_only(grad):
        clear()
        cs = [torch.rand((B, h, w, c), device="cuda", generator=g).requires_grad_(grad) for (h, w), c in zip(C_SIZES, C_WIDTHS)]
        ps = fpn(cs)
        torch.autograd.backward(ps, [torch.ones_like(p) for p in ps])

    def backbone_only(backbone):
        clear(backbone)
        cs = backbone(images)
        torch.autograd.backward(cs, [torch.ones_like(c) for c in cs])

    def step(backbone):
        clear(backbone)
        eb, cp = head(fpn(backbone(images)))
        out = ssd_amd.differentiable_loss(cp, eb, anchors, gt, {"gamma": 2.0, "alpha": 0.25})
        (out["localization_loss"] + out["classification_loss"]).backward()
    if train_first is None:
        t0, t1 = timed(lambda: fpn_only(False), reps), timed(lambda: fpn_only(True), reps)
        print("  the FPN alone, forward + backward: frozen features %8.2f ms, with the bridge to c3, c4, c5 %8.2f ms (+ %.2f ms)" % (t0, t1, t1 - t0))
        backbone = ssd_amd.TrainableMobileNet(params, W, device="cuda").train()
        timed_line("  the backbone alone (Conv2d_0 frozen; forward + backward of 26 convolutions and 26 batch norms) ", lambda: backbone_only(backbone))
        timed_line("  %s " % STEP, lambda: step(backbone))
        return
    res = {}
    for first in train_first:
        backbone = ssd_amd.TrainableMobileNet(params, W, device="cuda", train_first=first).train()
        for what, fn in ((BACKBONE, backbone_only), (STEP, step)):
            res[(what, first)] = timed_line("  train_first=%-5s  %-58s" % (first, what), lambda: fn(backbone))
        del backbone
    for what in sorted((STEP, BACKBONE)):
        print("  train_first on - off: %-58s %+8.2f ms" % (what, res[(what, True)] - res[(what, False)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), "| exact-fp32 MFMA peak %.1f TFLOP/s" % PEAK)
    for B in a.frames:
        print("%d frames of 640 x 896" % B)
        depthwise_lines("Conv2d_1", B, 320, 448, 32, 1, a.reps)
        depthwise_lines("Conv2d_2", B, 320, 448, 64, 2, a.reps)
        depthwise_lines("Conv2d_7", B, 40, 56, 512, 1, a.reps)
        pointwise_lines(B, 40, 56, 512, 512, a.reps)
        pointwise_lines(B, 20, 28, 1024, 1024, a.reps)
        bn_lines(B, 320, 448, 64, a.reps)
        bn_lines(B, 40, 56, 512, a.reps)
        torch.cuda.empty_cache()
        if not a.no_step:
            step_lines(B, max(1, a.reps // 2))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
