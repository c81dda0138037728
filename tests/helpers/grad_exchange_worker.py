"""Child process of tests/test_train_reduce_host.py (task 'digest', no GPU) and tests/test_gpu_trainer_distributed.py: one rank
of a data-parallel Trainer, or the one-process runs it is compared with.
    python grad_exchange_worker.py TASK WORKDIR
The rank comes from RANK / WORLD_SIZE (set by the test, or by torch.distributed.run for task 'rccl1'); WORKDIR/config.json is the
Trainer's config (written by the test), states go to WORKDIR as .npz files and the exit status says whether the in-process
checks held."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SEED = 40
HEADER_FLOATS = 16


def init_gloo():
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    return dist.get_rank(), dist.get_world_size()


def state(ts):
    """Every variable, moving statistic, average and both slots of a TrainStep as host arrays, and global_step."""
    out = {"statistic " + n: s.detach().cpu().numpy() for n, s in ts.statistics.items()}
    for n in ts.names:
        m, v = ts.slots(n)
        out.update({"variable " + n: ts.parameters[n].detach().cpu().numpy(), "average " + n: ts.ema(n).cpu().numpy(),
                    "m " + n: m.cpu().numpy(), "v " + n: v.cpu().numpy()})
    out["global_step"] = np.int64(ts.global_step)
    return out


def dump(path, st):
    keys = sorted(st)
    np.savez(path, keys=np.array(json.dumps(keys)), **{"a%05d" % i: st[k] for i, k in enumerate(keys)})


def load(path):
    with np.load(path) as z:
        keys = json.loads(str(z["keys"]))
        return {k: z["a%05d" % i] for i, k in enumerate(keys)}


def same_state(a, b):
    """The keys that differ in a bit (dtype, shape or any element's bits)."""
    if set(a) != set(b):
        return sorted(set(a) ^ set(b))
    return [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]


def config(work, run):
    cfg = json.load(open(os.path.join(work, "config.json")))
    return dict(cfg, model_dir=os.path.join(work, run))


def digest(work):
    """Two gloo CPU ranks: equal tables pass; tables that differ (a count; which gradient is present) raise on BOTH ranks."""
    from ssd_amd import grad_exchange, train_calls
    rank, _world = init_gloo()
    cpu = torch.device("cpu")

    def table(counts, present):
        t = np.zeros(len(counts), train_calls.REDUCE_ROW_DTYPE)
        t["count"] = counts
        t["offset"] = train_calls.bucket_layout(counts)[0]
        t["data"] = [(0x1000 * (rank + 1) + 64 * i) if p else 0 for i, p in enumerate(present)]     # addresses differ, presence counts
        return t
    grad_exchange.agree_on_table(table([5, 7, 9], [1, 1, 0]), None, cpu)
    raised = 0
    for mine in (table([5, 7 + rank, 9], [1, 1, 0]), table([5, 7, 9], [1, 1, rank]), table([5, 7, 9][:3 - rank], [1, 1, 0][:3 - rank])):
        try:
            grad_exchange.agree_on_table(mine, None, cpu)
        except ValueError as e:
            assert "rank(s) [1]" in str(e), e
            raised += 1
    assert raised == 3, raised
    open(os.path.join(work, "digest_rank%d.ok" % rank), "w").write("raised %d\n" % raised)
    dist.destroy_process_group()


def rccl1(work):
    """torch.distributed.run --nproc-per-node 1: two steps of a Trainer with the world-1 RCCL group equal two steps of the plain one."""
    import ssd_amd
    device, backend = ssd_amd.init_node_process_group()
    assert backend == "nccl" and dist.get_world_size() == 1, backend
    plain = ssd_amd.Trainer(config(work, "plain"), device=device, seed=SEED, read_workers=2)
    assert plain.train(max_steps=2, log_every=1) == 2
    want = state(plain.train_step)
    del plain
    grouped = ssd_amd.Trainer(config(work, "grouped"), device=device, seed=SEED, read_workers=2, group=dist.group.WORLD)
    assert grouped._exchange is not None and grouped._exchange.on_device
    assert grouped.train(max_steps=2, log_every=1) == 2
    got = state(grouped.train_step)
    differ = same_state(got, want)
    assert not differ, differ[:5]
    assert int(got["global_step"]) == 2 and len(got) == 4 * len(grouped.train_step.names) + len(grouped.train_step.statistics) + 1
    logs = [[json.loads(l) for l in open(os.path.join(work, d, "train_log.jsonl"))] for d in ("plain", "grouped")]
    for a, b in zip(*logs):
        for k in ("step", "loss", "localization_loss", "classification_loss", "regularization_loss", "gradient_norm", "learning_rate"):
            assert a[k] == b[k], (k, a[k], b[k])
    dist.destroy_process_group()


def two(work):
    """One of two gloo ranks that share cuda:0: two steps, the state to WORKDIR/state_rank<r>.npz."""
    import ssd_amd
    rank, world = init_gloo()
    t = ssd_amd.Trainer(config(work, "run"), device=0, seed=SEED, read_workers=2, group=dist.group.WORLD)
    assert not t._exchange.on_device and t.world == 2
    assert t.train(max_steps=2, log_every=1) == 2
    dump(os.path.join(work, "state_rank%d.npz" % rank), state(t.train_step))
    json.dump(t.last, open(os.path.join(work, "last_rank%d.json" % rank), "w"))
    dist.destroy_process_group()


def emulate(work):
    """The two ranks' two steps in ONE process on one model: rank 0's batch, then rank 1's batch from the same start state, both
    slices packed, reduced, the update."""
    import ssd_amd
    from ssd_amd import train_calls, trainer
    from conftest import TINY_PARAMS
    from helpers import train_reduce_ref as ref
    cfg = config(work, "emulation")
    dev = torch.device("cuda", 0)
    W = {**trainer.warm_start_weights(cfg["pretrained_checkpoint"], TINY_PARAMS), **trainer.head_tower_weights(TINY_PARAMS, SEED)}
    backbone = ssd_amd.TrainableMobileNet(TINY_PARAMS, W, device="cuda", seed=SEED, train_first=True).train()
    fpn = ssd_amd.TrainableFPN(TINY_PARAMS, W, device="cuda", seed=SEED).train()
    head = ssd_amd.TrainableBoxPredictor(TINY_PARAMS, W, device="cuda", seed=SEED).train()
    variables = {**backbone.named_variables(), **fpn.named_variables(), **head.named_variables()}
    statistics = {**backbone.statistics(), **fpn.statistics(), **head.statistics()}
    ts = ssd_amd.TrainStep(variables, cfg, statistics, layout="tf", params=TINY_PARAMS, frozen={})
    gen = ssd_amd.AnchorGenerator()
    anchors = torch.from_numpy(gen(128, 128)).cuda()
    levels = tuple(int(n) for n in gen.num_anchors_per_feature_map)
    pipes = [ssd_amd.TrainPipeline(cfg["train_dataset"], cfg, seed=trainer.pipeline_seed(SEED, 0), read_workers=2, shard=(r, 2))
             for r in range(2)]
    tensors = list(variables.values()) + list(statistics.values())
    counts = [t.numel() for t in tensors]
    offsets, _P, slice_floats = ref.bucket_layout(counts)
    for _ in range(2):
        start = [s.clone() for s in statistics.values()]
        gathered = torch.empty((2, slice_floats), dtype=torch.float32, device=dev)
        for r in range(2):
            images, gt = next(pipes[r])
            with torch.no_grad():
                for s, s0 in zip(statistics.values(), start):
                    s.copy_(s0)
            for p in variables.values():
                p.grad = None
            eb, cp = head(fpn(backbone(images)))
            out = ssd_amd.differentiable_loss(cp, eb, anchors, gt, cfg, anchors_per_level=levels, per_image=True)
            loc, cls = out["localization_loss"], out["classification_loss"]
            (float(np.float32(cfg["localization_loss_weight"])) * loc + float(np.float32(cfg["classification_loss_weight"])) * cls).backward()
            table = np.zeros(len(tensors), train_calls.REDUCE_ROW_DTYPE)
            table["count"], table["offset"] = counts, offsets
            table["kind"] = [0] * len(variables) + [1] * len(statistics)
            table["data"] = [p.grad.data_ptr() for p in variables.values()] + [s.data_ptr() for s in statistics.values()]
            rows_host = torch.from_numpy(table.view(np.uint8).copy())
            rows_dev = rows_host.to(dev)
            header = torch.stack([out["per_image"][:, 2].sum(), loc.detach(), cls.detach()])
            train_calls.train_grad_pack(rows_host, rows_dev, header, gathered[r])
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        weights = torch.empty(2, dtype=torch.float32, device=dev)
        train_calls.train_grad_reduce(rows_host, rows_dev, gathered, losses, weights)     # into rank 1's gradients and the statistics
        ts.step()
    torch.cuda.synchronize()
    for p in pipes:
        p._gen.close()
    dump(os.path.join(work, "state_emulation.npz"), state(ts))
    json.dump({"localization_loss": float(losses[0]), "classification_loss": float(losses[1]), "weights": weights.cpu().tolist()},
              open(os.path.join(work, "last_emulation.json"), "w"))


def nan(work):
    """One of two gloo ranks: rank 1 alone plants a NaN in one variable; BOTH ranks stop at step 1, no checkpoint is written."""
    import ssd_amd
    from ssd_amd import trainer
    rank, _world = init_gloo()
    cfg = config(work, "run")
    t = ssd_amd.Trainer(cfg, device=0, seed=SEED, read_workers=2, group=dist.group.WORLD)
    if rank == 1:
        with torch.no_grad():
            t.variables["box_net/encoded_boxes/bias"][5] = float("nan")
    try:
        t.train(max_steps=3, log_every=1)
    except FloatingPointError as e:
        assert str(e).startswith("step 1: "), e
        open(os.path.join(work, "stopped_rank%d.txt" % rank), "w").write(str(e))
    else:
        raise AssertionError("rank %d trained on" % rank)
    dist.barrier()
    assert trainer.checkpoint_steps(cfg["model_dir"]) == []
    dist.destroy_process_group()


if __name__ == "__main__":
    {"digest": digest, "rccl1": rccl1, "two": two, "emulate": emulate, "nan": nan}[sys.argv[1]](sys.argv[2])
