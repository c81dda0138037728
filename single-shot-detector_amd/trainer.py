"""train.py's loop (train.py:36-66, model.py:106-128 in mode TRAIN) without TensorFlow: the Trainer wires the pieces this library
already has --

    TrainPipeline -> TrainableMobileNet | TrainableShuffleNet (train_first) -> TrainableFPN -> TrainableBoxPredictor
                  -> differentiable_loss -> backward -> TrainStep.norms() -> TrainStep.step()

-- decides the start state as tf.estimator does (resume from model_dir, else warm-start the backbone from pretrained_checkpoint),
reports total_loss with the regularisation term from the GPU's per-tensor sums, stops on a non-finite loss, gradient or variable
(NanTensorHook), writes checkpoints and logs on a schedule and evaluates the moving averages (RestoreMovingAverageHook).

TensorBoard's event files (summaries.py: the scalars and a histogram of every variable and gradient, model.py:88-90, 113, 121-123)
are written every save_summary_steps steps, off by default in the API.  No graph capture of a step, no gradient clipping,
exact fp32 only.  With `group` the ranks of a process group train in lockstep, one GPU each
(grad_exchange.py).  The host
logic that needs no GPU -- schedules, seeds, the warm start, pruning, the stop decision -- is the module-level functions below.
"""
import json
import math
import os
import re
import time

import numpy as np

from .ckpt_import import read_checkpoint, read_checkpoint_index, resolve_checkpoint
from .config import (load_config, load_loss_config, load_optimizer_config, load_run_config, load_train_config)

SAVE_CHECKPOINTS_SECS = 1800            # train.py:39
EVAL_THROTTLE_SECS = 3 * 3600           # train.py:63
KEEP_CHECKPOINT_MAX = 5                 # tf.estimator.RunConfig's default
SAVE_SUMMARY_STEPS = 600                # train.py:39 (the command's default; the API's is 0: no summaries)
# the scalar tags of the reference's graph (model.py:88-90, 113 under variable_scope('learning_rate'); `loss` and `global_step/sec`
# are tf.estimator's own) -> the key of log_record that holds the value
SUMMARY_SCALARS = (("loss", "loss"), ("regularization_loss", "regularization_loss"), ("localization_loss", "localization_loss"),
                   ("classification_loss", "classification_loss"), ("learning_rate/learning_rate", "learning_rate"))
BACKBONE_SCOPES = {"mobilenet": "MobilenetV1/", "shufflenet": "ShuffleNetV2/"}     # train.py:44-47
GROUP_TIME_CHECK_STEPS = 100            # with a group, a schedule in seconds is examined at these steps only, by rank 0's clock
RING = 4                                # read-back slots: step k - 1 is examined after step k was enqueued


# ----------------------------------------------------------------------------- host logic
def due(step, now, last_step, last_time, every_steps, every_secs):
    """Is a scheduled action (a checkpoint, an evaluation) due after `step` at time `now`, the last one having happened after
    `last_step` at `last_time`?  every_steps (None: no step schedule) wins over every_secs (None: no time schedule), as in
    tf.estimator's CheckpointSaverHook, which takes exactly one of the two; never twice for one step."""
    if step <= last_step:
        return False
    if every_steps is not None:
        return step - last_step >= int(every_steps)
    if every_secs is not None:
        return now - last_time >= float(every_secs)
    return False


MATCHES_SCOPE = "losses/loss_summaries/"                                           # ssd.py:86, 125


def summary_due(step, last_summary_step, every):
    """SummarySaverHook's schedule: is a summary due at `step`, the last one of this (re)started run having been written at
    `last_summary_step` (None: none yet)?  The first step of a run, then every step with step - last >= every; every == 0: never."""
    every = int(every)
    if every < 0:
        raise ValueError("save_summary_steps must be >= 0")
    if every == 0:
        return False
    return last_summary_step is None or int(step) - int(last_summary_step) >= every


def summary_scalars(record, steps_per_second=None, per_image=None):
    """{tag: value} of one summary event from a log_record: SUMMARY_SCALARS, `global_step/sec` when a rate is known, and -- from
    ssd_loss's per_image rows [B, 3 + levels] -- the matches summaries of ssd.py:125-129, 154-163 under their name scopes: the
    mean over the batch of the matches per image, on each level (3 ..) and in total, float32 (a sum of small integers, one division)."""
    out = {tag: record[key] for tag, key in SUMMARY_SCALARS}
    if steps_per_second is not None:
        out["global_step/sec"] = float(steps_per_second)
    if per_image is not None:
        rows = np.asarray(per_image, np.float32)
        B = np.float32(rows.shape[0])
        for level in range(rows.shape[1] - 3):
            out[MATCHES_SCOPE + "mean_matches_per_image_on_level_%d" % (3 + level)] = float(rows[:, 3 + level].sum(dtype=np.float32) / B)
        out[MATCHES_SCOPE + "total_mean_matches_per_image"] = float(rows[:, 2].sum(dtype=np.float32) / B)
    return out


def pipeline_seed(seed, step):
    """The TrainPipeline seed of a run (re)started at global_step `step`: the entropy [seed, step], of which TrainPipeline makes
    SeedSequence([seed, step]), so that a resumed run does not replay the records the interrupted one began with (tf.estimator
    restarts its input on resume, too)."""
    if int(seed) < 0 or int(step) < 0:
        raise ValueError("seed and step must be >= 0")
    return [int(seed), int(step)]


def backbone_names(params):
    """The variables train.py's WarmStartSettings restores: those of variables.variable_shapes(params) under the backbone's scope."""
    from .variables import variable_shapes
    scope = BACKBONE_SCOPES[load_config(params)["backbone"]]
    return {n: tuple(s) for n, s in variable_shapes(params).items() if n.startswith(scope)}


def warm_start_weights(prefix, params):
    """{name: float32 array} of exactly backbone_names(params) out of the checkpoint `prefix` (a prefix, one of its files or a
    model_dir).  Whatever else the checkpoint holds -- a classifier's Logits, slots, averages -- is ignored; a missing backbone
    variable is a KeyError naming it, a wrong shape a ValueError."""
    found = resolve_checkpoint(prefix)
    if found is None:
        raise FileNotFoundError("pretrained_checkpoint %r is not a checkpoint prefix or model_dir" % (prefix,))
    want = backbone_names(params)
    _, entries = read_checkpoint_index(found)
    for name in want:
        if name not in entries:
            raise KeyError("pretrained checkpoint %s has no variable %r" % (found, name))
    got = read_checkpoint(found, list(want))
    out = {}
    for name, shape in want.items():
        a = got[name]
        if a.dtype != np.float32 or tuple(a.shape) != shape:
            raise ValueError("pretrained variable %r has shape %s dtype %s, expected %s float32" % (name, tuple(a.shape), a.dtype, shape))
        out[name] = np.ascontiguousarray(a)
    return out


def head_tower_weights(params, seed):
    """What box_predictor.py:107-155 initialises besides class_net/logits (which TrainableBoxPredictor draws itself): the towers'
    kernels by tf.variance_scaling_initializer (fpn_train.variance_scaling_draw), their batch norms (gamma 1, beta 0, moving_mean 0,
    moving_variance 1) and box_net/encoded_boxes (normal(0, 0.01), bias 0), in variables.variable_shapes order from ONE generator
    seeded by SeedSequence([seed, 1])."""
    from .fpn_train import variance_scaling_draw
    from .head_train import head_variable_shapes
    rng = np.random.default_rng(np.random.SeedSequence([int(seed), 1]))
    out = {}
    for name, shape in head_variable_shapes(params).items():
        if name.startswith("class_net/logits/"):
            continue
        leaf = name.rsplit("/", 1)[1]
        if name.startswith("box_net/encoded_boxes/"):
            a = rng.normal(0.0, 0.01, shape) if leaf == "kernel" else np.zeros(shape)
        elif leaf == "kernel":
            a = variance_scaling_draw(rng, shape)
        else:
            a = np.ones(shape) if leaf in ("gamma", "moving_variance") else np.zeros(shape)
        out[name] = np.asarray(a, np.float32)
    return out


def checkpoint_steps(model_dir):
    """The steps N of the complete bundles model.ckpt-N in model_dir, ascending."""
    if not os.path.isdir(model_dir):
        return []
    steps = []
    for f in os.listdir(model_dir):
        m = re.match(r"^model\.ckpt-(\d+)\.index$", f)
        if m:
            steps.append(int(m.group(1)))
    return sorted(steps)


def prune_checkpoints(model_dir, keep=KEEP_CHECKPOINT_MAX):
    """Deletes all but the newest `keep` bundles model.ckpt-N of model_dir (tf.train.Saver's max_to_keep); the `checkpoint` state
    file, which names the newest, is left alone.  Returns the removed prefixes."""
    if keep < 1:
        raise ValueError("keep must be >= 1")
    removed = []
    for step in checkpoint_steps(model_dir)[:-keep]:
        base = "model.ckpt-%d" % step
        for f in os.listdir(model_dir):
            if f == base + ".index" or re.match("^" + re.escape(base) + r"\.data-\d{5}-of-\d{5}$", f):
                os.remove(os.path.join(model_dir, f))
        removed.append(os.path.join(model_dir, base))
    return removed


def first_non_finite(step, names, loc, cls, sums, bad):
    """NanTensorHook's decision on one step's read-back (host values): None when everything is finite, else the message of the
    FloatingPointError, which names the step and the first offending variable -- the first row of `names` with a non-finite element
    in the variable, else in a gradient (bad [T,2]: a non-zero count; sums [T,2]: a non-finite sum, the squares overflowed) -- and, when
    every row is clean, the loss term that is not finite."""
    sums, bad = np.asarray(sums, np.float64), np.asarray(bad, np.int64)
    wrong = (bad != 0) | ~np.isfinite(sums)
    for col, what in ((0, "variable"), (1, "the gradient of")):                  # a bad variable is the cause, bad gradients follow
        rows = np.nonzero(wrong[:, col])[0]
        if len(rows):
            t = int(rows[0])
            if bad[t, col]:
                return "step %d: %s %r has %d non-finite element(s)" % (step, what, names[t], int(bad[t, col]))
            return "step %d: the sum of squares of %s %r is %r" % (step, what, names[t], float(sums[t, col]))
    for what, v in (("localization_loss", loc), ("classification_loss", cls)):
        if not math.isfinite(float(v)):
            return "step %d: %s is %r" % (step, what, float(v))
    return None


def log_record(step, loc, cls, reg, sums, loss_config, learning_rate, images_per_second, wait_seconds):
    """One train_log.jsonl record: loss is evaluation.total_loss's rule (tf.losses.get_total_loss) with the regularisation term."""
    from .evaluation import total_loss
    return {"step": int(step), "loss": float(total_loss(loc, cls, reg, loss_config)), "localization_loss": float(np.float32(loc)),
            "classification_loss": float(np.float32(cls)), "regularization_loss": float(np.float32(reg)),
            "learning_rate": float(learning_rate), "gradient_norm": float(math.sqrt(float(np.sum(np.asarray(sums, np.float64)[:, 1])))),
            "images_per_second": float(images_per_second), "wait_seconds": float(wait_seconds)}


def _append_jsonl(path, record):
    with open(path, "a") as f:
        f.write(json.dumps(record, sort_keys=True) + "\n")


# ----------------------------------------------------------------------------- the Trainer
class Trainer:
    """tf.estimator.Estimator(model_fn, params, config, warm_start_from) + train_and_evaluate of train.py on one GPU, or with `group`
    on one GPU per rank.

    config          the reference's JSON (path or dict): every key group of config.py is read from it
    model_dir       overrides the config's
    device          the HIP device index
    seed            the run's seed: the initial FPN and heads, and (with global_step at the start) the input pipeline
    read_workers, decode    TrainPipeline's (and evaluation.evaluate's)
    group           None: one process, one GPU | a torch.distributed process group: data-parallel training over its G ranks, one
                    process per GPU, every rank built with the same config, model_dir and seed.  The config's batch_size is PER
                    RANK: a step sees G x batch_size images, and initial_learning_rate is used as given (scaling it with G is the
                    user's decision).  The pipeline keeps shards[rank::G]; after backward() ONE all-gather exchanges the gradients,
                    the moving statistics and the loss terms (GradientExchange): the loss is the reference's over the global batch
                    (normalised by the matches of all ranks), batch statistics stay per replica and the moving statistics are
                    averaged.  Norms, histograms, the non-finite stop and the update see the reduced values, which are the same
                    bits on every rank; only rank 0 writes checkpoints, logs and event files (the matches summaries are rank
                    0's), and a barrier follows every save.  A group of one rank equals group=None bit for bit.
    metric_device   evaluation.evaluate's: None computes the AP of evaluate() on the host, a device computes it on that GPU

    Start state: a checkpoint in model_dir resumes the run (variables, statistics, averages, slots, global_step: TrainStep.restore);
    otherwise the backbone comes from pretrained_checkpoint (warm_start_weights) and fpn/* and the heads are drawn from `seed`.
    Every variable is trained (train_first, nothing frozen), as the reference does.

    step() never waits for the device on its own account: a step's loss terms, sums and counts go to one of RING pinned slots behind
    an event, and the host examines step k - 1's slot after it has enqueued step k (at most two slots are in flight)."""

    log_every = 100

    def __init__(self, config, model_dir=None, device=0, seed=0, read_workers=None, decode=None, group=None, metric_device=None):
        import torch
        from .backbone_train import TrainableMobileNet
        from .fpn_train import TrainableFPN
        from .head_train import TrainableBoxPredictor
        from .shufflenet_train import TrainableShuffleNet
        from .ssd import AnchorGenerator
        from .train_step import TrainStep
        if isinstance(config, dict):
            self.config = dict(config)
        else:
            with open(config) as f:
                self.config = json.load(f)
        self.params = load_config(self.config)
        self.loss_config = load_loss_config(self.config)
        self.train_config = load_train_config(self.config)
        self.run_config = load_run_config(self.config)
        load_optimizer_config(self.config)
        self.model_dir = str(model_dir if model_dir is not None else self.run_config["model_dir"])
        self.device = torch.device("cuda", int(device))
        self.seed = int(seed)
        self.read_workers, self.decode = read_workers, decode
        self.group = group
        self.metric_device = metric_device
        self.rank, self.world = 0, 1
        if group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        os.makedirs(self.model_dir, exist_ok=True)
        resumed = resolve_checkpoint(self.model_dir)
        if resumed is not None:
            from .ckpt_import import load_ckpt_weights
            W = load_ckpt_weights(resumed, self.params, use_ema=False)
        else:
            W = {**warm_start_weights(self.run_config["pretrained_checkpoint"], self.params), **head_tower_weights(self.params, self.seed)}
        backbone_cls = TrainableMobileNet if self.params["backbone"] == "mobilenet" else TrainableShuffleNet
        with torch.cuda.device(self.device):
            self.backbone = backbone_cls(self.params, W, device=self.device, seed=self.seed, train_first=True).train()
            self.fpn = TrainableFPN(self.params, W, device=self.device, seed=self.seed).train()
            self.head = TrainableBoxPredictor(self.params, W, device=self.device, seed=self.seed).train()
            self.variables = {**self.backbone.named_variables(), **self.fpn.named_variables(), **self.head.named_variables()}
            statistics = {**self.backbone.statistics(), **self.fpn.statistics(), **self.head.statistics()}
            self.train_step = TrainStep(self.variables, self.config, statistics, layout="tf", params=self.params, frozen={})
            if resumed is not None:
                self.train_step.restore(resumed)
            self._exchange = None
            if group is not None:
                from .grad_exchange import GradientExchange
                self._exchange = GradientExchange(self.train_step, statistics, group)
            gen = AnchorGenerator()
            hw = (self.train_config["image_height"], self.train_config["image_width"])
            self.anchors = torch.from_numpy(gen(*hw)).to(self.device)
            self.anchors_per_level = tuple(int(n) for n in gen.num_anchors_per_feature_map)
            self.loc_weight = torch.tensor(np.float32(self.loss_config["localization_loss_weight"]), device=self.device)
            self.cls_weight = torch.tensor(np.float32(self.loss_config["classification_loss_weight"]), device=self.device)
            T = len(self.train_step.names)
            self._ring = [{"losses": torch.empty(2, dtype=torch.float32).pin_memory(), "sums": torch.empty((T, 2), dtype=torch.float64).pin_memory(),
                           "bad": torch.empty((T, 2), dtype=torch.int64).pin_memory(), "event": torch.cuda.Event(), "step": None}
                          for _ in range(RING)]
        self.resumed_from = resumed
        self.start_step = self.train_step.global_step
        self._pipe = None
        self._pending = []                  # ring slots whose read-back the host has not examined, oldest first
        self._failed = False
        self._saved_step = self.start_step if resumed is not None else -1
        self._last_save = (self.start_step, time.monotonic())
        self._last_log = (self.start_step, time.monotonic())
        self.save_summary_steps = 0         # train()'s option: 0 enqueues, allocates and writes nothing
        self._last_summary = None           # the last step of THIS run with a summary
        self._last_rate = None              # (step, time) of the last summary event: global_step/sec
        self._hist_ring = None              # pinned read-back slots of the histograms, made by the first due step
        self.loss_histograms = False        # train()'s option: off enqueues, allocates and writes nothing
        self._loss_top = None               # the per-level top losses' buffers and table, made by the first due step that wants them
        self._writers = {}                  # logdir -> summaries.EventFileWriter
        self.last = None                    # the newest examined step's log_record

    @property
    def global_step(self):
        return self.train_step.global_step

    # ------------------------------------------------------------------ one step
    def _pipeline(self):
        if self._pipe is None:
            from .augment import TrainPipeline
            shard = None if self.group is None else (self.rank, self.world)
            self._pipe = TrainPipeline(self.run_config["train_dataset"], self.train_config, pipeline_seed(self.seed, self.global_step),
                                       decode=self.decode, read_workers=self.read_workers, device=self.device.index, shard=shard)
        return self._pipe

    def step(self):
        """Enqueues one training step and returns its number; examines the read-back of the step before it (FloatingPointError)."""
        import torch
        from .ssd import differentiable_loss
        if self._failed:
            raise RuntimeError("this run stopped on a non-finite value")
        with torch.cuda.device(self.device):
            images, gt = next(self._pipeline())
            for p in self.variables.values():
                p.grad = None
            eb, cp = self.head(self.fpn(self.backbone(images)))
            want_summary = summary_due(self.global_step + 1, self._last_summary, self.save_summary_steps)
            want_top = want_summary and self.loss_histograms and self.rank == 0
            if want_top:                                        # ... and its per-anchor planes, of the same pass (ssd.py:135-152)
                out = differentiable_loss(cp, eb, self.anchors, gt, self.loss_config, anchors_per_level=self.anchors_per_level,
                                          per_image=True, per_anchor=True)
            elif want_summary or self._exchange is not None:    # the loss with its per-image rows: the matches per level (ssd.py:154-163)
                out = differentiable_loss(cp, eb, self.anchors, gt, self.loss_config, anchors_per_level=self.anchors_per_level,
                                          per_image=True)
            else:
                out = differentiable_loss(cp, eb, self.anchors, gt, self.loss_config)
            loc, cls = out["localization_loss"], out["classification_loss"]
            (self.loc_weight * loc + self.cls_weight * cls).backward()
            if self._exchange is not None:
                # this rank's matches and its two losses, on the device; what comes back is over the global batch, on every rank alike
                header = torch.stack([out["per_image"][:, 2].sum(), loc.detach(), cls.detach()])
                loc, cls, _weights = self._exchange.exchange(header)
            sums, bad = self.train_step.norms()         # before the update: of the variables this step computed with
            hist = top = None
            if want_summary:
                if self.rank == 0:
                    hist = self.train_step.histograms()     # beside the norms, of the same variables and gradients
                    top = self._loss_top_histograms(out["cls_losses"], out["loc_losses"]) if want_top else None
                self._last_summary = self.global_step + 1
            t = self.train_step.step()
            slot = self._ring[t % RING]
            slot["hist"] = None
            if hist is not None:
                if self._hist_ring is None:
                    self._hist_ring = [{"counts": torch.empty(hist[0].shape, dtype=torch.int64).pin_memory(),
                                        "stats": torch.empty(hist[1].shape, dtype=torch.uint8).pin_memory(),
                                        "per_image": torch.empty(out["per_image"].shape, dtype=torch.float32).pin_memory()}
                                       for _ in range(RING)]
                slot["hist"] = self._hist_ring[t % RING]
                slot["hist"]["counts"].copy_(hist[0], non_blocking=True)
                slot["hist"]["stats"].copy_(hist[1], non_blocking=True)
                slot["hist"]["per_image"].copy_(out["per_image"], non_blocking=True)
                slot["hist"]["has_top"] = top is not None
                if top is not None:
                    if "top_counts" not in slot["hist"]:
                        slot["hist"].update(top_counts=torch.empty(top[0].shape, dtype=torch.int64).pin_memory(),
                                            top_stats=torch.empty(top[1].shape, dtype=torch.uint8).pin_memory())
                    slot["hist"]["top_counts"].copy_(top[0], non_blocking=True)
                    slot["hist"]["top_stats"].copy_(top[1], non_blocking=True)
            slot["losses"][0:1].copy_(loc.detach().reshape(1), non_blocking=True)
            slot["losses"][1:2].copy_(cls.detach().reshape(1), non_blocking=True)
            slot["sums"].copy_(sums, non_blocking=True)
            slot["bad"].copy_(bad, non_blocking=True)
            slot["event"].record(torch.cuda.current_stream(self.device))
            slot["step"] = t
            self._pending.append(slot)
        while len(self._pending) > 1:                   # step t - 1 (and older), after step t was enqueued
            self._examine(self._pending[0])
        return t

    def _loss_top_histograms(self, cls_losses, loc_losses):
        """(counts, stats) of the ten `*_losses_on_level_*` histograms of this step (include/ssd_hip.h, "the per-level top losses"):
        ssd_loss_top_means into a persistent [2,K] buffer, then ssd_train_histograms over a table of 2 * L rows, row p * L + l the
        K-slice of plane p and level l (no gradient: only plane 0 of a row counts; m, v and ema point at the row itself, where the
        table's checks accept them, and are never dereferenced).  The buffers, the limits and the table are made and uploaded by the
        first call; every later call enqueues the five launches and nothing else."""
        import torch
        from . import train_calls
        from .train_step import TENSOR_DTYPE, block_starts
        if self._loss_top is None:
            counts = train_calls.loss_top_counts(self.anchors_per_level)
            L, K = len(counts), sum(counts)
            means = torch.empty((2, K), dtype=torch.float32, device=self.device)
            starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
            rows = np.zeros(2 * L, TENSOR_DTYPE)
            ptrs = np.array([means.data_ptr() + 4 * (p * K + int(starts[l])) for p in range(2) for l in range(L)], np.uint64)
            for field in ("w", "m", "v", "ema"):
                rows[field] = ptrs
            rows["count"] = np.tile(np.asarray(counts, np.int64), 2)
            rows["first_block"], _blocks = block_starts(ptrs, rows["count"])
            host = torch.from_numpy(rows.view(np.uint8).copy())
            limits = torch.from_numpy(train_calls.histogram_limits().copy()).to(self.device)
            self._loss_top = {"means": means, "host": host, "dev": host.to(self.device), "limits": limits,
                              "counts": torch.empty((2 * L, 2, limits.numel()), dtype=torch.int64, device=self.device),
                              "stats": torch.empty((2 * L, 2, train_calls.STATS_BYTES), dtype=torch.uint8, device=self.device)}
        top = self._loss_top
        train_calls.loss_top_means(cls_losses, loc_losses, self.anchors_per_level, top["means"])
        train_calls.train_histograms(top["host"], top["dev"], np.float32(0.0), top["limits"], top["counts"], top["stats"])
        return top["counts"], top["stats"]

    def _examine(self, slot):
        assert slot is self._pending[0]
        slot["event"].synchronize()
        self._pending.pop(0)
        step = slot["step"]
        loc, cls = (float(v) for v in slot["losses"].numpy())
        sums, bad = slot["sums"].numpy(), slot["bad"].numpy()
        msg = first_non_finite(step, self.train_step.names, loc, cls, sums, bad)
        if msg is not None:
            self._failed = True
            self._pending.clear()
            raise FloatingPointError(msg)
        reg = self.train_step.regularization_loss(sums)
        now = time.monotonic()
        images = (step - self._last_log[0]) * self.train_config["batch_size"] * self.world
        rate = images / max(now - self._last_log[1], 1e-9)
        self.last = log_record(step, loc, cls, reg, sums, self.loss_config, self.train_step.learning_rate(step - 1), rate,
                               self._pipe.wait_seconds if self._pipe is not None else 0.0)
        if self.log_every and step % self.log_every == 0:
            if self.rank == 0:
                _append_jsonl(os.path.join(self.model_dir, "train_log.jsonl"), self.last)
            self._last_log = (step, now)
        if slot.get("hist") is not None:
            try:
                self._write_summary(step, slot["hist"], now)
            except FloatingPointError:                  # g + weight_decay * w overflowed where g and w were finite: TF stops here, too
                self._failed = True
                self._pending.clear()
                raise

    def _writer(self, logdir):
        from .summaries import EventFileWriter
        if logdir not in self._writers:
            self._writers[logdir] = EventFileWriter(logdir)
        return self._writers[logdir]

    def _write_summary(self, step, hist, now):
        """The summary event of an examined, finite step: the scalars of its log_record and `<name>_hist` / `<name>_grad_hist` of
        every variable (a parameter without a gradient gets no `_grad_hist`)."""
        from .summaries import histogram_proto
        from .train_calls import STATS_DTYPE, histogram_limits
        limits = histogram_limits()
        counts = hist["counts"].numpy()
        stats = hist["stats"].numpy().view(STATS_DTYPE)[:, :, 0]
        histograms = {}
        for t, name in enumerate(self.train_step.names):
            histograms[name + "_hist"] = histogram_proto(limits, counts[t, 0], stats[t, 0])
            if stats[t, 1]["num"] > 0:
                histograms[name + "_grad_hist"] = histogram_proto(limits, counts[t, 1], stats[t, 1])
        if hist.get("has_top"):                         # ssd.py:135-152: row p * L + l of the table, plane 0
            top_counts = hist["top_counts"].numpy()
            top_stats = hist["top_stats"].numpy().view(STATS_DTYPE)[:, :, 0]
            L = top_counts.shape[0] // 2
            for p, kind in enumerate(("classification", "localization")):
                for l in range(L):
                    histograms[MATCHES_SCOPE + "%s_losses_on_level_%d" % (kind, 3 + l)] = \
                        histogram_proto(limits, top_counts[p * L + l, 0], top_stats[p * L + l, 0])
        rate = None
        if self._last_rate is not None and now > self._last_rate[1]:
            rate = (step - self._last_rate[0]) / (now - self._last_rate[1])
        self._last_rate = (step, now)
        self._writer(self.model_dir).add_summary(step, summary_scalars(self.last, rate, hist["per_image"].numpy()), histograms)

    def drain(self):
        """Examines every outstanding read-back (waits for the device)."""
        while self._pending:
            self._examine(self._pending[0])

    # ------------------------------------------------------------------ checkpoints, evaluation
    def save(self):
        """A checkpoint of the current step (after draining: none is written once a step was non-finite), the newest
        KEEP_CHECKPOINT_MAX kept.  Returns the prefix."""
        if self._failed:
            raise RuntimeError("this run stopped on a non-finite value")
        self.drain()
        if self.group is not None:
            prefix = self._save_in_group()
        else:
            prefix = self.train_step.save(self.model_dir)
            prune_checkpoints(self.model_dir, KEEP_CHECKPOINT_MAX)
        self._saved_step = self.global_step
        self._last_save = (self.global_step, time.monotonic())
        return prefix

    def _save_in_group(self):
        """save()'s write with a group: rank 0 writes and prunes, a barrier follows, every rank returns the prefix."""
        import torch.distributed as dist
        if self.rank == 0:
            self.train_step.save(self.model_dir)
            prune_checkpoints(self.model_dir, KEEP_CHECKPOINT_MAX)
        dist.barrier(group=self.group)
        return os.path.join(self.model_dir, "model.ckpt-%d" % self.global_step)

    def evaluate(self):
        """estimator.evaluate with RestoreMovingAverageHook: the moving averages of the current step's checkpoint over val_dataset;
        the dict (with `step`) is appended to model_dir/eval_log.jsonl and returned."""
        from .detector import Detector
        from .evaluation import evaluate
        if self._saved_step != self.global_step:
            self.save()
        self.drain()
        det = Detector(self.model_dir, visible_device_list=str(self.device.index), config=self.config, use_ema=True)
        try:
            res = evaluate(det, self.run_config["val_dataset"], self.config, read_workers=self.read_workers, decode=self.decode,
                           group=self.group, metric_device=self.metric_device)
        finally:
            det.close()
        res = dict(res, step=int(self.global_step))
        if self.rank != 0:
            return res
        _append_jsonl(os.path.join(self.model_dir, "eval_log.jsonl"), res)
        if self.save_summary_steps:
            scalars = {k: v for k, v in res.items() if k != "step" and isinstance(v, (int, float)) and not isinstance(v, bool)}
            self._writer(os.path.join(self.model_dir, "eval")).add_summary(int(self.global_step), scalars)
        return res

    def _due(self, step, last_step, last_time, every_steps, every_secs):
        """due() now, decided alike on every rank of the group: a schedule in steps needs no exchange; one in seconds is rank 0's
        decision, taken every GROUP_TIME_CHECK_STEPS steps and sent to the others (a save or an evaluation is a collective:
        ranks whose clocks disagree would wait for each other for ever)."""
        mine = due(step, time.monotonic(), last_step, last_time, every_steps, every_secs)
        if self.group is None or every_steps is not None:
            return mine
        if every_secs is None or step % GROUP_TIME_CHECK_STEPS:
            return False
        import torch
        import torch.distributed as dist
        from .distributed import _all_gather_ints
        small = self.device if dist.get_backend(self.group) == "nccl" else torch.device("cpu")
        return bool(_all_gather_ints([int(mine)], self.group, small)[0, 0])

    def train(self, max_steps=None, save_checkpoints_steps=None, save_checkpoints_secs=SAVE_CHECKPOINTS_SECS, log_every=100, on_step=None,
              save_summary_steps=0, loss_histograms=False):
        """Steps until global_step == max_steps (default num_steps), checkpoints on schedule and at the end.  on_step(step) is
        called after each enqueued step; when it returns True the loop ends early (train_and_evaluate's evaluations).
        save_summary_steps: 0 no summaries | n: model_dir/events.out.tfevents.* gets the scalars and the histograms of every variable
        and gradient at the run's first step and then every n steps (summary_due).
        loss_histograms: with summaries on, every summary event also gets the reference's ten `classification_losses_on_level_3..7`
        / `localization_losses_on_level_3..7` histograms (ssd.py:135-152; rank 0's batch under `group`): of each image the top 20 %
        of a level's per-anchor losses in descending order, averaged over the batch slot by slot (include/ssd_hip.h, "the per-level
        top losses": the set is the reference's, the slot order is this library's).  Off: nothing is enqueued, allocated or written."""
        max_steps = int(self.config["num_steps"] if max_steps is None else max_steps)
        self.log_every = int(log_every)
        summary_due(0, None, save_summary_steps)        # refuses a negative value
        self.save_summary_steps = int(save_summary_steps)
        self.loss_histograms = bool(loss_histograms)
        try:
            while self.global_step < max_steps:
                t = self.step()
                if self._due(t, self._last_save[0], self._last_save[1], save_checkpoints_steps,
                             None if save_checkpoints_steps is not None else save_checkpoints_secs):
                    self.save()
                if on_step is not None and on_step(t):
                    break
            self.drain()
            if self._saved_step != self.global_step:
                self.save()
        finally:
            self.close_pipeline()
        return self.global_step

    def train_and_evaluate(self, max_steps=None, eval_every_steps=None, eval_every_secs=EVAL_THROTTLE_SECS, save_checkpoints_steps=None,
                           save_checkpoints_secs=SAVE_CHECKPOINTS_SECS, log_every=100, on_eval=None, save_summary_steps=0,
                           loss_histograms=False):
        """tf.estimator.train_and_evaluate (train.py:61-66): trains, evaluates on schedule and once more at the end.  Returns the
        list of evaluation dicts; on_eval(dict) is called with each as it is made.  save_summary_steps, loss_histograms: train()'s; when set, every
        evaluation's scalar entries are also written to model_dir/eval/events.out.tfevents.* at its step."""
        max_steps = int(self.config["num_steps"] if max_steps is None else max_steps)
        summary_due(0, None, save_summary_steps)
        self.save_summary_steps = int(save_summary_steps)
        results = []
        last = [self.global_step, time.monotonic()]

        def on_step(t):
            if t < max_steps and self._due(t, last[0], last[1], eval_every_steps,
                                           None if eval_every_steps is not None else eval_every_secs):
                results.append(self.evaluate())
                if on_eval is not None:
                    on_eval(results[-1])
                last[0], last[1] = t, time.monotonic()
            return False
        self.train(max_steps, save_checkpoints_steps, save_checkpoints_secs, log_every, on_step, save_summary_steps, loss_histograms)
        results.append(self.evaluate())
        if on_eval is not None:
            on_eval(results[-1])
        return results

    def close_pipeline(self):
        """Stops the input pipeline's decode threads; the next step() starts a fresh one, seeded by the step it starts at."""
        if self._pipe is not None:
            gen, self._pipe = self._pipe._gen, None
            if gen is not None:
                gen.close()
