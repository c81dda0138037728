"""What one training step of the FPN costs (include/ssd_hip.h, "the TRAIN FPN"): per entry point, with HIP events, at 8 and 32
frames of 640 x 896 (c3, c4, c5 = 80x112, 40x56, 20x28; MobileNet widths 256, 512, 1024), num_classes 80.

    python scripts/fpn_train_cost.py [--frames 8 32] [--reps 5] [--no-step]

Reports the forward, data-gradient and weight-gradient time and TFLOP/s of lateral3 (1x1, 256 -> 256 at 80x112), p3 (3x3,
256 -> 256 at 80x112) and p6 (3x3 stride 2, 1024 -> 256 at 20x28 -> 10x14) against the 157.3 TFLOP/s exact-fp32 MFMA peak -- the
yardstick is the head's 256 -> 256 weight gradient at 0.52 of it --, the two forms of ssd_fpn_merge_backward in
GB/s, and one whole FPN + head step (forward, loss, backward) through TrainableFPN and TrainableBoxPredictor."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import train_calls as calls                          # noqa: E402
from head_train_cost import PEAK, SIZES, timed                    # noqa: E402

C_SIZES = [(80, 112), (40, 56), (20, 28)]
C_WIDTHS = [256, 512, 1024]


def conv_lines(name, B, H, W, Cin, Cout, k, stride, with_dx, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    OH, OW = -(-H // stride), -(-W // stride)
    x = torch.randn((B, H, W, Cin), device="cuda", generator=g)
    dy = torch.randn((B, OH, OW, Cout), device="cuda", generator=g)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    w = torch.randn((k, k, Cin, Cout), device="cuda", generator=g) * 0.05
    dw = torch.empty_like(w)
    ws = torch.empty(calls.conv_workspace_bytes([x], B, Cin, Cout, k, stride), dtype=torch.uint8, device="cuda")
    bwd = lambda dxs: calls.conv_backward([x], w, [dy], dw, stride, dxs, workspace=ws)
    fl = 2.0 * k * k * Cin * Cout * B * OH * OW
    tf = lambda t: fl / t / 1e9
    t_f = timed(lambda: calls.conv_forward([x], w, [y], stride, workspace=ws), reps)
    t_w = timed(lambda: bwd(None), reps)
    print("  %-9s %dx%d s%d %4d -> %3d at %dx%d  output rows %7d  workspace %6.1f MB" % (name, k, k, stride, Cin, Cout, H, W, B * OH * OW, ws.numel() / 1e6))
    print("    forward (permutes + pack + igemm)     %8.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_f, tf(t_f), 100 * tf(t_f) / PEAK))
    print("    weight gradient (wgrad + reduce)      %8.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_w, tf(t_w), 100 * tf(t_w) / PEAK))
    if with_dx:
        t_x = timed(lambda: bwd([dx]), reps)
        t_d = t_x - t_w
        # a stride-2 data gradient runs the launch over the zero-dilated gradient: stride^2 times the useful multiply-adds
        print("    data gradient (permutes + pack + igemm) %6.3f ms  %6.1f TFLOP/s useful  %4.1f %% of peak  (backward with dx %.3f ms minus the weight gradient)"
              % (t_d, tf(t_d), 100 * tf(t_d) / PEAK, t_x))
    else:
        print("    data gradient                         not needed: %s" % ("refused for 1x1" if k == 1 else "its input is the frozen backbone's"))


def merge_lines(B, reps, C=256):
    g = torch.Generator(device="cuda").manual_seed(2)
    H, W = 40, 56
    big, base = torch.randn((B, 2 * H, 2 * W, C), device="cuda", generator=g), torch.randn((B, H, W, C), device="cuda", generator=g)
    out = torch.empty_like(base)
    t = timed(lambda: ssd_amd.fpn_merge_backward(big, base=base, out=out), reps)
    nb = (big.numel() + 2 * base.numel()) * 4.0
    print("  merge backward, dx4 = dx4' + 2x2 sums of dx3 (%dx%d <- %dx%d)  %8.3f ms  %7.1f GB/s moved" % (H, W, 2 * H, 2 * W, t, nb / t / 1e6))
    p6 = torch.randn((B, 10, 14, C), device="cuda", generator=g)
    o6 = torch.empty_like(p6)
    t = timed(lambda: ssd_amd.fpn_merge_backward(p6, base=p6, gate=p6, same_size=True, out=o6), reps)
    print("  merge backward, gated same-size form (p6, 10x14)                  %8.3f ms  %7.1f GB/s moved" % (t, 4 * p6.numel() * 4.0 / t / 1e6))


def step_line(B, reps):
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
    W = ssd_amd.synthetic_weights(params, seed=1)
    fpn = ssd_amd.TrainableFPN(params, W, device="cuda").train()
    head = ssd_amd.TrainableBoxPredictor(params, W, device="cuda").train()
    g = torch.Generator(device="cuda").manual_seed(3)
    cs = [torch.rand((B, h, w, c), device="cuda", generator=g) for (h, w), c in zip(C_SIZES, C_WIDTHS)]
    anchors = torch.from_numpy(ssd_amd.AnchorGenerator()(640, 896)).cuda()
    boxes = np.tile(np.array([[[0.2, 0.2, 0.6, 0.7], [0.5, 0.1, 0.9, 0.4]]], np.float32), (B, 1, 1))
    gt = {"boxes": boxes, "labels": np.ones((B, 2), np.int32), "num_boxes": np.full(B, 2, np.int32)}

    def fpn_only():
        for p in fpn.parameters():
            p.grad = None
        ps = fpn(cs)
        torch.autograd.backward(ps, [torch.ones_like(p) for p in ps])

    def step():
        for p in list(fpn.parameters()) + list(head.parameters()):
            p.grad = None
        eb, cp = head(fpn(cs))
        out = ssd_amd.differentiable_loss(cp, eb, anchors, gt, {"gamma": 2.0, "alpha": 0.25})
        (out["localization_loss"] + out["classification_loss"]).backward()
    t0 = timed(fpn_only, reps)
    print("  the FPN alone (forward + backward of its ten convolutions and five batch norms, upstream gradient of ones)  %8.2f ms" % t0)
    torch.cuda.reset_peak_memory_stats()
    t = timed(step, reps)
    print("  one FPN + head step (forward + loss + backward, frozen c3 .. c5)  %8.2f ms  peak memory %.2f GB" % (t, torch.cuda.max_memory_allocated() / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), "| exact-fp32 MFMA peak %.1f TFLOP/s" % PEAK)
    assert SIZES[0] == C_SIZES[0]
    for B in a.frames:
        print("%d frames of 640 x 896" % B)
        conv_lines("lateral3", B, 80, 112, 256, 256, 1, 1, False, a.reps)
        conv_lines("p3", B, 80, 112, 256, 256, 3, 1, True, a.reps)
        conv_lines("p6", B, 20, 28, 1024, 256, 3, 2, False, a.reps)
        conv_lines("p7", B, 10, 14, 256, 256, 3, 2, True, a.reps)
        merge_lines(B, a.reps)
        if not a.no_step:
            step_line(B, max(1, a.reps // 2))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
