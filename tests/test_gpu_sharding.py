"""Mixed-size detection and both evaluations sharded over ranks, on the GPU: every rank a fresh child process under its own
time limit (never exec); two ranks share cuda:0 over gloo (at most three processes have the GPU open: the two ranks and
this one).  Results must not depend on the world size, the chunk size or which rank ran an image."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "helpers", "sharding_gpu_worker.py")
sys.path.insert(0, HERE)

from helpers import example_protos  # noqa: E402


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(task, work, world=None, timeout=300):
    """One-process run (world None) or `world` gloo ranks started together; every child's exit status must be 0."""
    if world is None:
        r = subprocess.run([sys.executable, WORKER, task, str(work)], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return
    port, procs = _port(), []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, task, str(work)], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)


@pytest.mark.gpu
def test_detect_many_sharded_two_ranks_one_gpu(cuda, tmp_path):
    """37 images of 10 sizes split 23 + 14: every rank gets every image's detections, bit-equal to detect_many."""
    _run("detect", tmp_path, world=2)


@pytest.mark.gpu
def test_detect_many_sharded_rccl_world1(cuda, tmp_path):
    """torch.distributed.run --nproc-per-node 1: backend nccl, records in device memory, the all-gather in place."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), WORKER, "rccl", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _jpeg_folder(work):
    from PIL import Image
    rng = np.random.default_rng(21)
    sizes = [(128, 128), (100, 150), (160, 120), (128, 256), (90, 200), (200, 130), (64, 300), (140, 141), (300, 90)]
    metas = []
    for k in range(22):
        h, w = sizes[k % len(sizes)]
        name = "im%02d.jpg" % k
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(work, name), quality=92)
        metas.append({"id": 1000 - 7 * k, "file_name": name, "height": h, "width": w})
    json.dump(metas, open(os.path.join(work, "images.json"), "w"))


@pytest.mark.gpu
def test_coco_eval_two_ranks_equals_one_process(cuda, tmp_path):
    _jpeg_folder(tmp_path)
    _run("coco1", tmp_path)
    _run("coco2", tmp_path, world=2)
    one = np.load(tmp_path / "stats_1.npy")
    assert one[0] > 0 and one[1] > one[0]
    for rank in range(2):
        assert np.array_equal(np.load(tmp_path / ("stats_2_rank%d.npy" % rank)), one)
    assert (tmp_path / "pred_2.json").read_bytes() == (tmp_path / "pred_1.json").read_bytes()


def _shard(work, n=19):
    sys.path.insert(0, ROOT)
    import ssd_amd
    os.makedirs(os.path.join(work, "shard"), exist_ok=True)
    rng = np.random.default_rng(4)
    sizes = [(128, 128), (100, 150), (160, 120), (128, 256), (90, 200), (200, 130), (128, 128), (140, 300)]
    records = []
    for k in range(n):
        h, w = sizes[k % len(sizes)]
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = int(rng.integers(0, 5))
        lo = rng.uniform(0.0, 0.5, (m, 2))
        hi = lo + rng.uniform(0.1, 0.5, (m, 2))
        boxes = np.clip(np.concatenate([lo, hi], 1), 0, 1).astype(np.float32)
        records.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, m)))
    ssd_amd.tfrecords.write_records(os.path.join(work, "shard", "val-00000.tfrecords"), records)


@pytest.mark.gpu
def test_evaluation_two_ranks_equals_one_process(cuda, tmp_path):
    _shard(tmp_path)
    _run("eval1", tmp_path)
    _run("eval2", tmp_path, world=2)
    one = json.load(open(tmp_path / "eval1_rank0.json"))
    assert one["num_images"] == 19 and one["classification_loss"] > 0
    for rank in range(2):
        assert json.load(open(tmp_path / ("eval2_rank%d.json" % rank))) == one


@pytest.mark.gpu
def test_evaluation_cli_gpus2_prints_the_gpus1_line(cuda, tmp_path):
    import ssd_amd
    _shard(tmp_path, n=11)
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 3, "score_threshold": 0.15, "iou_threshold": 0.6,
              "max_boxes_per_class": 25, "min_dimension": 128, "gamma": 2.0, "alpha": 0.25, "localization_loss_weight": 1.0,
              "classification_loss_weight": 2.0, "weight_decay": 5e-5}
    ssd_amd.save_weights(str(tmp_path / "w.npz"), ssd_amd.synthetic_weights(params, seed=3, logits_bias=-1.0))
    json.dump(params, open(tmp_path / "config.json", "w"))
    lines = []
    for n in (1, 2):
        cmd = [sys.executable, "-m", "ssd_amd.evaluation", str(tmp_path / "w.npz"), "--config", str(tmp_path / "config.json"),
               "--val_dataset", str(tmp_path / "shard"), "--max_batch", "4", "--gpus", str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout                  # printed once, by rank 0
        lines.append(out[0])
    assert lines[1] == lines[0]
    assert json.loads(lines[0])["num_images"] == 11


@pytest.mark.gpu
def test_loss_rows_do_not_depend_on_the_batch(ssd, cuda):
    """The per-image ssd_loss row (and predictions) of an image are the same whatever its companions, the batch size and
    the batch's groundtruth padding G -- what lets any rank run any image."""
    import ssd_amd.evaluation  # noqa: F401
    params = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 3, "score_threshold": 0.15, "iou_threshold": 0.6,
              "max_boxes_per_class": 25, "min_dimension": 128}
    eng = ssd.Engine(params, ssd.synthetic_weights(params, seed=7, logits_bias=-1.0), device=0, precision="f32")
    rng = np.random.default_rng(12)
    sizes = [(128, 128), (100, 100), (90, 90), (140, 140), (64, 64), (200, 200)]     # one network shape: 128 x 128
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    gts = []
    for k in range(len(frames)):
        m = [2, 0, 5, 1, 9, 3][k]
        lo = rng.uniform(0.0, 0.5, (m, 2))
        gts.append((np.clip(np.concatenate([lo, lo + rng.uniform(0.1, 0.5, (m, 2))], 1), 0, 1).astype(np.float32),
                    rng.integers(0, 3, m)))
    lc = {"gamma": 2.0, "alpha": 0.25}
    run = ssd.evaluation._Run(eng)
    alone = [run([f], [g], lc)[0] for f, g in zip(frames, gts)]
    for order in ([0, 1, 2, 3, 4, 5], [5, 3, 0], [2, 4], [1, 0, 5, 4, 3, 2], [4, 4, 0, 1]):
        got = run([frames[i] for i in order], [gts[i] for i in order], lc)
        for i, g in zip(order, got):
            a = alone[i]
            assert np.array_equal(g[0], a[0]) and np.array_equal(g[1], a[1])
            assert all(np.array_equal(u, v) for u, v in zip(g[2], a[2]))
    assert any(a[0][2] > 0 for a in alone)            # some images have matches
    eng.close()
