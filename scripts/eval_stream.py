"""The evaluation module over the val2017-like stream of scripts/val_like_stream.py (its sizes; frames as decoded arrays,
so no JPEG decode is timed).  usage: python scripts/eval_stream.py [n_images]
Under `python -m torch.distributed.run --nproc-per-node N scripts/eval_stream.py [n_images]` the images shard over the N ranks
(evaluate(..., group)); rank 0 prints."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, ssd_amd, bench
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
P = bench.PARAMS
cfg = dict(P, gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0, weight_decay=5e-5)
group, device, rank = None, 0, 0
if "WORLD_SIZE" in os.environ:
    import torch.distributed as dist
    device, backend = ssd_amd.init_node_process_group()
    group, rank = dist.group.WORLD, dist.get_rank()
det = ssd_amd.Detector(ssd_amd.synthetic_weights(P, seed=0, logits_bias=-7.5), config=cfg, visible_device_list=str(device))
common = [(480, 640)] * 24 + [(640, 480)] * 7 + [(427, 640)] * 12 + [(640, 427)] * 4 + [(375, 500)] * 6 + [(500, 375)] * 2 + [(426, 640)] * 5 + [(428, 640)] * 3 + \
         [(425, 640)] * 2 + [(424, 640)] * 2 + [(640, 426)] * 2 + [(333, 500)] * 3 + [(500, 333)] * 1 + [(360, 640)] * 2 + [(480, 480)] + [(612, 612)] * 2 + [(640, 640)] * 2
tail = [(400, 600), (512, 640), (640, 512), (478, 640), (359, 640), (500, 400), (640, 359), (281, 500), (500, 281), (213, 640), (640, 213), (300, 400), (240, 320),
        (320, 240), (453, 640), (640, 453), (383, 640), (536, 640), (640, 536), (429, 640), (361, 640), (500, 334), (332, 500), (464, 640), (595, 640), (375, 640)]
rng = np.random.default_rng(0)
sizes = [common[i] for i in rng.integers(0, len(common), n - n // 8)] + [tail[i] for i in rng.integers(0, len(tail), n // 8)]
rng.shuffle(sizes)
data = []
for h, w in sizes:
    k = int(rng.integers(1, 8))
    lo = rng.uniform(0, 0.7, (k, 2)); hi = lo + rng.uniform(0.05, 0.3, (k, 2))
    data.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.concatenate([lo, hi], 1).astype(np.float32), rng.integers(0, 80, k)))
for rnd in range(2):
    t0 = time.perf_counter()
    res = ssd_amd.evaluation.evaluate(det, data, cfg, max_batch=32, group=group)
    dt = time.perf_counter() - t0
    if rank == 0:
        print("world %d, " % (1 if group is None else dist.get_world_size()) + "pass %d (%s): %d images in %.2f s = %.0f img/s; %s" % (rnd, "plans built on the way" if rnd == 0 else "plans cached", n, dt, n / dt, res), flush=True)
if group is not None:
    dist.destroy_process_group()
