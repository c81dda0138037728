"""What one training step of the detection head costs (include/ssd_hip.h, "the TRAIN head"): per entry point, with HIP events, at
8 and 32 frames of 640 x 896 (p3 .. p7 = 80x112 .. 5x7), num_classes 80.

    python scripts/head_train_cost.py [--frames 8 32] [--reps 5] [--no-step] [--no-torch]

Reports TFLOP/s of the forward, data-gradient and weight-gradient launches against the 157.3 TFLOP/s exact-fp32 MFMA peak, GB/s of
the batch-norm calls (bytes they actually move: forward 3 reads + 1 write of the tensor, backward 4 reads + 1 write), one whole
head step (forward, loss, backward) through TrainableBoxPredictor, and -- when torch's own convolution backward runs on this GPU
-- F.conv2d forward + backward on the same shapes as a second reference line.  For the per-kernel view run it once under
`rocprofv3 --kernel-trace --stats -- python scripts/head_train_cost.py --frames 8 --reps 1 --no-torch`."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch                                                      # noqa: E402
import ssd_amd                                                    # noqa: E402
from ssd_amd import train_calls as calls                          # noqa: E402

PEAK = 157.3
SIZES = [(80, 112), (40, 56), (20, 28), (10, 14), (5, 7)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def conv_lines(B, Cin, Cout, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn((B, h, w, Cin), device="cuda", generator=g) for h, w in SIZES]
    dys = [torch.randn((B, h, w, Cout), device="cuda", generator=g) for h, w in SIZES]
    ys = [torch.empty_like(d) for d in dys]
    dxs = [torch.empty_like(x) for x in xs]
    w = torch.randn((3, 3, Cin, Cout), device="cuda", generator=g) * 0.05
    dw, db = torch.empty_like(w), torch.empty(Cout, device="cuda")
    ws = torch.empty(calls.conv_workspace_bytes(SIZES, B, Cin, Cout, entry="conv3x3"), dtype=torch.uint8, device="cuda")
    bwd = lambda dxs_, db_: calls.conv_backward(xs, w, dys, dw, dxs=dxs_, dbias=db_, workspace=ws, entry="conv3x3")
    R = B * sum(h * w for h, w in SIZES)
    fl = 2.0 * 9 * Cin * Cout * R
    t_f = timed(lambda: calls.conv_forward(xs, w, ys, workspace=ws, entry="conv3x3"), reps)
    t_w = timed(lambda: bwd(None, None), reps)
    t_x = timed(lambda: bwd(dxs, None), reps)
    t_b = timed(lambda: bwd(dxs, db), reps)
    tf = lambda t: fl / t / 1e9
    print("  conv %3d -> %3d  rows %7d  workspace %6.1f MB" % (Cin, Cout, R, ws.numel() / 1e6))
    print("    forward (permutes + pack + igemm)     %8.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_f, tf(t_f), 100 * tf(t_f) / PEAK))
    print("    weight gradient (wgrad + reduce)      %8.3f ms  %6.1f TFLOP/s  %4.1f %% of peak" % (t_w, tf(t_w), 100 * tf(t_w) / PEAK))
    t_d = t_x - t_w                                              # both calls without dbias: the difference is the data gradient alone
    print("    data gradient (permutes + pack + igemm) %6.3f ms  %6.1f TFLOP/s  %4.1f %% of peak  (backward with dx %.3f ms minus the weight gradient)"
          % (t_d, tf(t_d), 100 * tf(t_d) / PEAK, t_x))
    print("    dbias (2 launches)                    %8.3f ms  (backward with dx and dbias %.3f ms minus backward with dx)" % (t_b - t_x, t_b))


def bn_lines(B, reps, C=256):
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn((B, h, w, C), device="cuda", generator=g) for h, w in SIZES]
    dys = [torch.randn_like(x) for x in xs]
    outs = [torch.empty_like(x) for x in xs]
    par = torch.ones((5, 9, C), device="cuda")
    gamma, beta, mm, mv, mean, var, invstd, dgamma, dbeta = [[par[i, k] for i in range(5)] for k in range(9)]
    ws = torch.empty(calls.bn_workspace_bytes(xs, C), dtype=torch.uint8, device="cuda")
    t_f = timed(lambda: calls.bn_forward(xs, outs, gamma, beta, True, 1e-3, 0.007, mm, mv, mean, var, invstd, workspace=ws, entry="bn_relu"), reps)
    t_b = timed(lambda: calls.bn_backward(xs, dys, outs, gamma, beta, mean, invstd, dgamma, dbeta, workspace=ws, entry="bn_relu"), reps)
    nbytes = sum(x.numel() for x in xs) * 4.0
    print("  batch norm + relu, 5 levels, C = %d, tensor %.1f MB" % (C, nbytes / 1e6))
    print("    forward  (5 launches, 4 passes)       %8.3f ms  %7.1f GB/s moved" % (t_f, 4 * nbytes / t_f / 1e6))
    print("    backward (3 launches, 5 passes)       %8.3f ms  %7.1f GB/s moved" % (t_b, 5 * nbytes / t_b / 1e6))


def step_line(B, reps):
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
    W = ssd_amd.synthetic_weights(params, seed=1)
    m = ssd_amd.TrainableBoxPredictor(params, W, device="cuda").train()
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = [torch.randn((B, h, w, 256), device="cuda", generator=g) for h, w in SIZES]
    anchors = torch.from_numpy(ssd_amd.AnchorGenerator()(640, 896)).cuda()
    boxes = np.tile(np.array([[[0.2, 0.2, 0.6, 0.7], [0.5, 0.1, 0.9, 0.4]]], np.float32), (B, 1, 1))
    gt = {"boxes": boxes, "labels": np.ones((B, 2), np.int32), "num_boxes": np.full(B, 2, np.int32)}

    def step():
        for p in m.parameters():
            p.grad = None
        eb, cp = m(feats)
        out = ssd_amd.differentiable_loss(cp, eb, anchors, gt, {"gamma": 2.0, "alpha": 0.25})
        (out["localization_loss"] + out["classification_loss"]).backward()
    t = timed(step, reps)
    fl = 3 * 2.0 * 9 * 256 * (8 * 256 + 24 + 480) * B * sum(h * w for h, w in SIZES) - 2 * 2.0 * 9 * 256 * 256 * B * sum(h * w for h, w in SIZES)
    print("  one head step (forward + loss + backward, frozen p3 .. p7: no dx below the first tower layers)  %8.2f ms  %6.1f TFLOP/s  peak memory %.2f GB"
          % (t, fl / t / 1e9, torch.cuda.max_memory_allocated() / 1e9))


def torch_line(B, reps):
    import torch.nn.functional as F
    try:
        xs = [torch.randn((B, 256, h, w), device="cuda", requires_grad=True) for h, w in SIZES]
        w = (torch.randn((256, 256, 3, 3), device="cuda") * 0.05).requires_grad_()

        def run():
            for x in xs:
                x.grad = None
            w.grad = None
            sum(F.conv2d(x, w, padding=1).sum() for x in xs).backward()
        t = timed(run, reps)
        fl = 3 * 2.0 * 9 * 256 * 256 * B * sum(h * w for h, w in SIZES)
        print("  torch F.conv2d 256 -> 256 forward + backward (NCHW, its own kernels, tf32 off)  %8.3f ms  %6.1f TFLOP/s" % (t, fl / t / 1e9))
    except Exception as e:                                         # noqa: BLE001
        print("  torch F.conv2d backward did not run on this GPU: %r" % (e,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    print("device:", torch.cuda.get_device_name(0), "| exact-fp32 MFMA peak %.1f TFLOP/s" % PEAK)
    for B in a.frames:
        print("%d frames of 640 x 896" % B)
        for cin, cout in ((256, 256), (256, 24), (256, 480)):
            conv_lines(B, cin, cout, a.reps)
        bn_lines(B, a.reps)
        if not a.no_torch:
            torch_line(B, a.reps)
        if not a.no_step:
            step_line(B, max(1, a.reps // 2))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
