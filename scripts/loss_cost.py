"""A 32-frame 640x896 batch through the forward, then its loss (ssd_loss): per-step milliseconds by HIP events.
usage: rocprofv3 --kernel-trace --stats -- python scripts/loss_cost.py"""
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
anchors_np = g(640, 896)
anchors = torch.from_numpy(anchors_np).cuda()
N, C = len(anchors_np), P["num_classes"]
G = 100
boxes = np.zeros((B, G, 4), np.float32)
for b in range(B):
    lo = rng.uniform(0, 0.7, (G, 2)); hi = lo + rng.uniform(0.02, 0.3, (G, 2))
    boxes[b] = np.concatenate([lo, hi], 1)
gt = {"boxes": torch.from_numpy(boxes).cuda(), "labels": torch.from_numpy(rng.integers(0, 80, (B, G)).astype(np.int32)).cuda(),
      "num_boxes": torch.from_numpy(rng.integers(1, G + 1, B).astype(np.int32)).cuda()}
logits = torch.empty((B, N, C), device="cuda"); codes = torch.empty((B, N, 4), device="cuda")
def step():
    eng.forward(x)
    eng.get_tensor_dev("class_predictions", (B, N, C)); eng.get_tensor_dev("encoded_boxes", (B, N, 4))
for _ in range(3):
    step()
lg = eng.get_tensor_dev("class_predictions", (B, N, C)); cd = eng.get_tensor_dev("encoded_boxes", (B, N, 4))
for _ in range(3):
    ssd_amd.ssd_loss(lg, cd, anchors, gt, anchors_per_level=g.num_anchors_per_feature_map)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
fw, ls = [], []
for _ in range(10):
    ev[0].record(); eng.forward(x); ev[1].record()
    l, per = ssd_amd.ssd_loss(lg, cd, anchors, gt, anchors_per_level=g.num_anchors_per_feature_map); ev[2].record()
    torch.cuda.synchronize()
    fw.append(ev[0].elapsed_time(ev[1])); ls.append(ev[1].elapsed_time(ev[2]))
print("B=%d 640x896 N=%d C=%d G<=%d: forward %.2f ms (median of 10), loss %.3f ms (median, incl. workspace alloc + host->device gt copy) = %.1f %% of the step"
      % (B, N, C, G, np.median(fw), np.median(ls), 100 * np.median(ls) / (np.median(fw) + np.median(ls))))
print("losses", l.cpu().numpy().tolist(), "matches per image (first 4)", per[:4, 2].cpu().numpy().tolist())
