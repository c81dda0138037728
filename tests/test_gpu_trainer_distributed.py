"""ssd_amd.Trainer over the ranks of a process group, on the GPU: every rank a fresh child process under its own
time limit (never exec); two ranks share cuda:0 over gloo (at most three processes have the GPU open: the two ranks and this
one).  test_gpu_trainer.py's tiny config at 128 x 128, batch 2 per rank, on two 12-record training shards."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from helpers import example_protos
from helpers.grad_exchange_worker import load, same_state
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "helpers", "grad_exchange_worker.py")
BASE = dict(TINY_PARAMS, batch_size=2, image_height=128, image_width=128, initial_learning_rate=1e-3, num_steps=100, weight_decay=1e-4,
            gamma=2.0, alpha=0.25, localization_loss_weight=1.0, classification_loss_weight=2.0)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard(path, n, seed):
    """n JPEGs of random sizes with 1 .. 3 boxes each (test_gpu_trainer.py's writer)."""
    from ssd_amd import tfrecords
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        H, W = int(rng.integers(90, 260)), int(rng.integers(90, 260))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        m = int(rng.integers(1, 4))
        c = rng.uniform(0.1, 0.6, (m, 2))
        boxes = np.concatenate([c, c + rng.uniform(0.15, 0.35, (m, 2))], 1).clip(0, 1)
        recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, m)))
    tfrecords.write_records(path, recs)


@pytest.fixture(scope="module")
def data(ssd, tmp_path_factory):
    """Two training shards (one per rank at world 2), a validation shard and a pretrained MobileNet checkpoint."""
    from ssd_amd import ckpt_export
    root = tmp_path_factory.mktemp("trainer_distributed")
    os.makedirs(root / "train")
    os.makedirs(root / "val")
    _shard(str(root / "train" / "train-00.tfrecords"), 12, 0)
    _shard(str(root / "train" / "train-01.tfrecords"), 12, 2)
    _shard(str(root / "val" / "val-00.tfrecords"), 4, 1)
    W = ssd.synthetic_weights(TINY_PARAMS, seed=301, logits_bias=-4.0)
    ckpt = {k: v for k, v in W.items() if k.startswith("MobilenetV1/")}
    return dict(BASE, train_dataset=str(root / "train"), val_dataset=str(root / "val"),
                pretrained_checkpoint=ckpt_export.write_checkpoint(str(root / "pretrained.ckpt"), ckpt))


def _work(data, tmp_path):
    json.dump(dict(data, model_dir=str(tmp_path / "unused")), open(tmp_path / "config.json", "w"))
    return str(tmp_path)


def _ranks(task, work, world=2, timeout=300):
    """`world` gloo ranks started together, each a child under its own time limit; every exit status must be 0."""
    port, procs = _port(), []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, task, work], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
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


def test_rccl_world1_equals_the_plain_trainer(cuda, data, tmp_path):
    """torch.distributed.run --nproc-per-node 1: backend nccl, the slice packed in place, the all-gather in device memory; two steps
    with the group equal two steps without it in every variable, statistic, average, both slots and global_step (the worker)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), WORKER, "rccl1", _work(data, tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(tmp_path / "grouped" / "model.ckpt-2.index")


def test_two_ranks_equal_each_other_and_a_one_process_emulation(cuda, data, tmp_path):
    work = _work(data, tmp_path)
    _ranks("two", work)
    r = subprocess.run([sys.executable, WORKER, "emulate", work], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    states = [load(tmp_path / ("state_rank%d.npz" % rank)) for rank in range(2)]
    want = load(tmp_path / "state_emulation.npz")
    assert int(want["global_step"]) == 2 and len(want) > 4 * 100
    assert not same_state(states[0], states[1]), same_state(states[0], states[1])[:5]
    assert not same_state(states[0], want), same_state(states[0], want)[:5]
    # what the ranks report of step 2 is the same, and its losses are the emulation's reduced ones
    last = [json.load(open(tmp_path / ("last_rank%d.json" % rank))) for rank in range(2)]
    emu = json.load(open(tmp_path / "last_emulation.json"))
    for k in ("step", "loss", "localization_loss", "classification_loss", "regularization_loss", "gradient_norm", "learning_rate"):
        assert last[0][k] == last[1][k], k
    assert last[0]["step"] == 2 and last[0]["localization_loss"] == emu["localization_loss"]
    assert last[0]["classification_loss"] == emu["classification_loss"]
    assert len(emu["weights"]) == 2 and 0 < min(emu["weights"]) and abs(sum(emu["weights"]) - 1) < 1e-6
    # only rank 0 wrote: ONE checkpoint of step 2, one log with the two steps
    run = tmp_path / "run"
    assert sorted(f for f in os.listdir(run) if f.startswith("model.ckpt")) == ["model.ckpt-2.data-00000-of-00001", "model.ckpt-2.index"]
    assert [json.loads(l)["step"] for l in open(run / "train_log.jsonl")] == [1, 2]
    assert sorted(os.listdir(run)) == ["checkpoint", "model.ckpt-2.data-00000-of-00001", "model.ckpt-2.index", "train_log.jsonl"]


def test_a_nan_on_one_rank_stops_both(cuda, data, tmp_path):
    work = _work(data, tmp_path)
    _ranks("nan", work)
    msgs = [open(tmp_path / ("stopped_rank%d.txt" % rank)).read() for rank in range(2)]
    assert "variable 'box_net/encoded_boxes/bias' has 1 non-finite" in msgs[1]         # the rank that holds the NaN
    # the other rank sees it in what the exchange brought: the reduced loss (rank 1's is NaN), or a reduced gradient
    assert msgs[0].startswith("step 1: ") and ("localization_loss is nan" in msgs[0] or "the gradient of" in msgs[0]), msgs[0]
    assert not [f for f in os.listdir(tmp_path / "run") if f.startswith(("model.ckpt", "checkpoint"))]


def test_cli_gpus2_trains_two_steps_and_rank0_writes(cuda, data, tmp_path):
    """python -m ssd_amd.train --gpus 2 as typed: launch_local starts two ranks (gloo: they share the one GPU); ONE log with the two
    steps and ONE checkpoint of step 2 are left, written by rank 0."""
    import ssd_amd
    json.dump(dict(data, model_dir=str(tmp_path / "run")), open(tmp_path / "config.json", "w"))
    cmd = [sys.executable, "-m", "ssd_amd.train", "--config", str(tmp_path / "config.json"), "--gpus", "2", "--max_steps", "2",
           "--save_checkpoints_steps", "2", "--log_every", "1", "--seed", "40", "--no_eval", "--save-summary-steps", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = tmp_path / "run"
    log = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert [rec["step"] for rec in log] == [1, 2] and all(np.isfinite(v) for rec in log for v in rec.values())
    assert sorted(os.listdir(run)) == ["checkpoint", "model.ckpt-2.data-00000-of-00001", "model.ckpt-2.index", "train_log.jsonl"]
    saved = ssd_amd.read_checkpoint(ssd_amd.resolve_checkpoint(str(run)), ["global_step", "box_net/encoded_boxes/bias"])
    assert int(saved["global_step"]) == 2 and np.isfinite(saved["box_net/encoded_boxes/bias"]).all()
