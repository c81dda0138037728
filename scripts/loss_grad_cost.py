"""The gradient of the loss of a 32-frame 640x896 step (ssd_loss_backward) beside its forward loss (ssd_loss): per-call
milliseconds by HIP events and the logits bytes moved per second.
usage: rocprofv3 --kernel-trace --stats -- python scripts/loss_grad_cost.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, ssd_amd, bench
P = bench.PARAMS
B = 32
eng = ssd_amd.Engine(P, ssd_amd.synthetic_weights(P, seed=0, logits_bias=-4.0), device=0, precision="f32")
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.integers(0, 256, (B, 640, 896, 3), dtype=np.uint8)).cuda()
g = ssd_amd.AnchorGenerator()
anchors = torch.from_numpy(g(640, 896)).cuda()
N, C = int(anchors.shape[0]), P["num_classes"]
G = 100
boxes = np.zeros((B, G, 4), np.float32)
for b in range(B):
    lo = rng.uniform(0, 0.7, (G, 2)); hi = lo + rng.uniform(0.02, 0.3, (G, 2))
    boxes[b] = np.concatenate([lo, hi], 1)
gt = {"boxes": torch.from_numpy(boxes).cuda(), "labels": torch.from_numpy(rng.integers(0, 80, (B, G)).astype(np.int32)).cuda(),
      "num_boxes": torch.from_numpy(rng.integers(1, G + 1, B).astype(np.int32)).cuda()}
eng.forward(x)
lg = eng.get_tensor_dev("class_predictions", (B, N, C)); cd = eng.get_tensor_dev("encoded_boxes", (B, N, 4))
levels = g.num_anchors_per_feature_map
reg, cls, m = ssd_amd.get_training_targets(anchors, gt["boxes"], gt["labels"], gt["num_boxes"])
grad = torch.tensor([1.0, 1.0], device="cuda")
for _ in range(3):
    losses, per = ssd_amd.ssd_loss(lg, cd, anchors, gt, anchors_per_level=levels)
    d_l, d_c = ssd_amd.ssd_loss_backward(lg, cd, reg, cls, m, per, grad_losses=grad)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
fw, bw = [], []
for _ in range(10):
    ev[0].record()
    losses, per = ssd_amd.ssd_loss(lg, cd, anchors, gt, anchors_per_level=levels); ev[1].record()
    d_l, d_c = ssd_amd.ssd_loss_backward(lg, cd, reg, cls, m, per, grad_losses=grad); ev[2].record()
    torch.cuda.synchronize()
    fw.append(ev[0].elapsed_time(ev[1])); bw.append(ev[1].elapsed_time(ev[2]))
nbytes = 2 * B * N * C * 4 + 2 * B * N * 16
print("B=%d 640x896 N=%d C=%d G<=%d: ssd_loss %.3f ms, ssd_loss_backward %.3f ms (medians of 10, each incl. its output "
      "allocation) = %.2f TB/s of logits + gradients + codes (%.0f MB)"
      % (B, N, C, G, np.median(fw), np.median(bw), nbytes / np.median(bw) / 1e9, nbytes / 1e6))
print("losses", losses.cpu().numpy().tolist(), "|d_logits| sum %.6g, |d_codes| sum %.6g, nonfinite %d"
      % (d_l.abs().sum().item(), d_c.abs().sum().item(), int((~torch.isfinite(d_l)).sum().item())))
