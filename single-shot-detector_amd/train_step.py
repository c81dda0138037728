"""train.py's train_op after the gradients (model.py:106-128): cosine-decayed Adam with the weight-decay term's gradient, the
exponential moving average (EMA) of every trainable variable, and the checkpoint that carries the result back into this library
(`Detector(model_dir)`, `load_ckpt_weights(..., use_ema=True)`, `python -m ssd_amd.evaluation`).

The arithmetic is single-sourced in include/ssd_hip.h, block "the TRAIN update": the host half (learning rate, step size and EMA
decay, float64, each rounded once) is `step_scalars` here, the per-element half is ONE launch of csrc/update.hip over every tensor
of the model.  The caller's torch model and torch autograd produce the gradients (`differentiable_loss`); backward through the
network and the batch-norm statistics' own updates are the caller's.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib
from .ckpt_export import write_checkpoint, write_checkpoint_state
from .ckpt_import import EMA_SUFFIX, read_checkpoint, read_checkpoint_index, resolve_checkpoint
from .config import load_optimizer_config

BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8            # tf.train.AdamOptimizer's defaults (model.py:116 passes the rate only)
ONE_MINUS_BETA1, ONE_MINUS_BETA2 = 0.1, 0.001       # what the kernel receives, as float32
MOVING_AVERAGE_DECAY = 0.993                        # model.py:10
BLOCK_ELEMS = 4096                                  # SSD_UPDATE_BLOCK_ELEMS
# ssd_update_tensor of include/ssd_hip.h
TENSOR_DTYPE = np.dtype([("w", "<u8"), ("grad", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"), ("count", "<i8"),
                         ("decay", "<i4"), ("first_block", "<i4")])
assert TENSOR_DTYPE.itemsize == ctypes.sizeof(_lib.SsdUpdateTensor) == 56
_STATISTICS = ("moving_mean", "moving_variance")


def decays(name):
    """add_weight_decay's selection (model.py:132-145) on a variable name."""
    return ("weights" in name or "kernel" in name) and "depthwise_weights" not in name


def trainable_names(params):
    """The names of variables.variable_shapes(params) that tf.trainable_variables() holds: all but the batch-norm statistics."""
    from .variables import variable_shapes
    return [n for n in variable_shapes(params) if n.rsplit("/", 1)[1] not in _STATISTICS]


def learning_rate(config, global_step):
    """tf.train.cosine_decay(initial_learning_rate, global_step, num_steps) in float64 (model.py:108-113); global_step is the
    value BEFORE the update (t - 1)."""
    n = config["num_steps"]
    return config["initial_learning_rate"] * 0.5 * (1.0 + math.cos(math.pi * min(int(global_step), n) / n))


def ema_decay(num_updates):
    """ExponentialMovingAverage's decay with num_updates (model.py:126-127); num_updates is global_step AFTER the update (t)."""
    return min(MOVING_AVERAGE_DECAY, (1.0 + num_updates) / (10.0 + num_updates))


def step_scalars(config, t):
    """The six float32 scalars of update number t = 1, 2, ... as an _lib.SsdUpdateScalars."""
    lr = float(np.float32(learning_rate(config, t - 1)))
    alpha = lr * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    return _lib.SsdUpdateScalars(alpha, ONE_MINUS_BETA1, ONE_MINUS_BETA2, EPSILON, config["weight_decay"], 1.0 - ema_decay(t))


def block_starts(w_ptrs, counts):
    """first_block of every row and the total (include/ssd_hip.h): a tensor's blocks are counted from the 16-byte boundary at or
    below w."""
    blocks = (np.asarray(counts, np.int64) + ((np.asarray(w_ptrs, np.uint64) >> np.uint64(2)) & np.uint64(3)).astype(np.int64)
              + (BLOCK_ELEMS - 1)) // BLOCK_ELEMS
    ends = np.cumsum(blocks)
    return ends - blocks, int(ends[-1])


def to_tf_layout(name, a):
    """A torch-layout array as the TF variable: OIHW -> HWIO, a depthwise [C,1,k,k] -> [k,k,C,1]; everything else as it is."""
    if a.ndim != 4:
        return a
    return np.ascontiguousarray(a.transpose(2, 3, 0, 1) if "depthwise_weights" in name else a.transpose(2, 3, 1, 0))


def from_tf_layout(name, a):
    """The inverse of to_tf_layout."""
    if a.ndim != 4:
        return a
    return np.ascontiguousarray(a.transpose(2, 3, 0, 1) if "depthwise_weights" in name else a.transpose(3, 2, 0, 1))


class TableRing:
    """RING pinned slots for a table that changes from call to call: each slot is a pinned host buffer (`bytes`: its NumPy view), a
    device twin and the event of its last upload.  Call k takes slot k mod RING, so a slot is rewritten only after the upload that
    read it RING calls ago has run; until then nobody waits for the device.

    device, dtype, T   the device of the twins, the NumPy dtype of one row and the number of rows"""

    RING = 4

    def __init__(self, device, dtype, T, slots=RING):
        import torch
        self.device = device
        self.calls = 0
        self.slots = []
        with torch.cuda.device(device):
            for _ in range(slots):
                host = torch.empty(T * dtype.itemsize, dtype=torch.uint8).pin_memory()
                self.slots.append({"host": host, "bytes": host.numpy(), "dev": torch.empty(host.numel(), dtype=torch.uint8, device=device),
                                   "event": torch.cuda.Event()})

    def upload(self, rows, stream=None):
        """This call's rows (an array of the ring's dtype) into the next slot and, asynchronously on the current stream of the
        device (`stream`, where the caller holds it already), into its twin -> the slot's (host, dev) tensors for ssd_train_update
        or train_calls.*.  Waits only for the upload that last read this slot."""
        slot = self.slots[self.calls % len(self.slots)]
        if self.calls >= len(self.slots):
            slot["event"].synchronize()          # the upload that last read this pinned slot (RING calls ago) has run
        slot["bytes"][:] = rows.view(np.uint8)   # as bytes (another length raises): NumPy copies a structured array field by field
        slot["dev"].copy_(slot["host"], non_blocking=True)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        slot["event"].record(stream)
        self.calls += 1
        return slot["host"], slot["dev"]

    def last(self):
        """(host, dev) of the latest upload: valid until RING - 1 further calls."""
        slot = self.slots[(self.calls - 1) % len(self.slots)]
        return slot["host"], slot["dev"]


class TrainStep:
    """The optimizer state of one model and its update.

    named_parameters   {reference variable name (variables.variable_shapes): float32 CUDA leaf tensor}, contiguous, all on one device
    config             a path or dict with OPTIMIZER_KEYS (load_optimizer_config)
    statistics         {`.../moving_mean` | `.../moving_variance` name: float32 tensor}: never updated here, only carried by save / restore
    layout             "torch": parameters are OIHW (depthwise [C,1,k,k]) and are transposed to TF's HWIO ([k,k,C,1]) on save and back on
                       restore; "tf": parameters already have the variables' shapes
    params             the inference config (backbone, depth_multiplier, num_classes): when given, every name must be one of
                       variable_shapes(params) with that shape (in TF layout)
    frozen             {reference variable name: float32 array in TF layout} of variables that are NOT trained (a frozen backbone):
                       never read by step(); save writes them as they are, without averages or slots, so that the checkpoint
                       holds the whole model; restore leaves them alone

    m, v and ema live in three flat allocations of this object (`slots(name)`, `ema(name)` are views in the parameter's shape and
    layout); m and v start at 0, ema as a copy of the parameter.  `step()` is one kernel launch behind one small asynchronous
    upload and never waits for the device."""

    RING = TableRing.RING

    def __init__(self, named_parameters, config, statistics=None, layout="torch", params=None, frozen=None):
        import torch
        if layout not in ("torch", "tf"):
            raise ValueError("layout must be 'torch' or 'tf'")
        self.config = load_optimizer_config(config)
        self.layout = layout
        items = list(named_parameters.items()) if hasattr(named_parameters, "items") else list(named_parameters)
        if not items:
            raise ValueError("TrainStep needs at least one parameter")
        names = [n for n, _ in items]
        if len(set(names)) != len(names):
            raise ValueError("duplicate parameter name")
        shapes = None
        if params is not None:
            from .variables import variable_shapes
            shapes = variable_shapes(params)
        device = None
        for name, p in items:
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
                raise TypeError("parameter %r must be a float32 torch tensor" % name)
            if not p.is_cuda:
                raise ValueError("parameter %r is not on a GPU (there is no CPU update)" % name)
            if device is None:
                device = p.device
            if p.device != device:
                raise ValueError("parameter %r is on %s, the others on %s" % (name, p.device, device))
            if not p.is_leaf or not p.is_contiguous() or p.numel() < 1 or p.data_ptr() % 4:
                raise ValueError("parameter %r must be a non-empty contiguous leaf tensor" % name)
            if shapes is not None:
                if name not in shapes or name.rsplit("/", 1)[1] in _STATISTICS:
                    raise KeyError("%r is not a trainable variable of this architecture (variables.variable_shapes)" % name)
                if self._tf_shape(name, p.shape) != tuple(shapes[name]):
                    raise ValueError("parameter %r has shape %s in layout %r, the variable %s" % (name, tuple(p.shape), layout, shapes[name]))
        spans = sorted((p.data_ptr(), p.data_ptr() + 4 * p.numel(), n) for n, p in items)
        for (_a0, a1, an), (b0, _b1, bn) in zip(spans, spans[1:]):
            if b0 < a1:
                raise ValueError("parameters %r and %r share storage" % (an, bn))
        self.statistics = dict(statistics or {})
        for name, s in self.statistics.items():
            if not isinstance(s, torch.Tensor) or s.dtype != torch.float32:
                raise TypeError("statistic %r must be a float32 torch tensor" % name)
            if name.rsplit("/", 1)[-1] not in _STATISTICS or name in names:
                raise KeyError("%r is not a moving_mean / moving_variance name" % name)
            if shapes is not None and (name not in shapes or tuple(s.shape) != tuple(shapes[name])):
                raise KeyError("statistic %r is not a variable of this architecture with shape %s" % (name, tuple(s.shape)))
        self.frozen = {}
        for name, a in (frozen or {}).items():
            if name in names or name in self.statistics:
                raise KeyError("frozen variable %r is also a parameter or a statistic" % name)
            a = np.ascontiguousarray(a, dtype=np.float32)
            if shapes is not None and (name not in shapes or tuple(a.shape) != tuple(shapes[name])):
                raise KeyError("frozen variable %r is not a variable of this architecture with shape %s" % (name, a.shape))
            self.frozen[name] = a
        self.names = names
        self.parameters = dict(items)
        self.device = device
        self.global_step = 0
        self._index = {n: i for i, n in enumerate(names)}
        T = len(items)
        counts = np.array([p.numel() for _, p in items], np.int64)
        self._w_ptrs = np.array([p.data_ptr() for _, p in items], np.uint64)
        # a tensor's m, v and ema start at its w's offset inside a 16-byte group, so that the kernel's 16-byte path applies
        pad = ((self._w_ptrs >> np.uint64(2)) & np.uint64(3)).astype(np.int64)
        offsets = np.zeros(T, np.int64)
        cursor = 0
        for i in range(T):
            offsets[i] = cursor + pad[i]
            cursor = (offsets[i] + counts[i] + 3) // 4 * 4
        with torch.cuda.device(device):
            self._m = torch.zeros(cursor, dtype=torch.float32, device=device)
            self._v = torch.zeros(cursor, dtype=torch.float32, device=device)
            self._ema = torch.zeros(cursor, dtype=torch.float32, device=device)
            self._views = []
            for i, (_n, p) in enumerate(items):
                sl = slice(int(offsets[i]), int(offsets[i] + counts[i]))
                views = tuple(b[sl].view(p.shape) for b in (self._m, self._v, self._ema))
                views[2].copy_(p.detach())
                self._views.append(views)
            table = np.zeros(T, TENSOR_DTYPE)
            table["w"] = self._w_ptrs
            for k, col in enumerate(("m", "v", "ema")):
                table[col] = [vw[k].data_ptr() for vw in self._views]
            table["count"] = counts
            table["decay"] = [1 if decays(n) else 0 for n in names]
            table["first_block"], self.blocks = block_starts(self._w_ptrs, counts)
            self._table = table
        self._ring = TableRing(device, TENSOR_DTYPE, T)
        self._norms_ring = self._hist_ring = self._hist_limits = None       # made by the first norms() / histograms()
        _lib.lib()

    def _tf_shape(self, name, shape):
        shape = tuple(shape)
        if self.layout == "tf" or len(shape) != 4:
            return shape
        return (shape[2], shape[3], shape[0], shape[1]) if "depthwise_weights" in name else (shape[2], shape[3], shape[1], shape[0])

    # ------------------------------------------------------------------ state
    def slots(self, name):
        """(m, v) of the parameter `name`: views into this object's flat buffers."""
        return self._views[self._index[name]][:2]

    def ema(self, name):
        """The moving average of the parameter `name`: a view into this object's flat buffer."""
        return self._views[self._index[name]][2]

    def learning_rate(self, step):
        """The learning rate (float64) of the update that starts at global_step == step."""
        return learning_rate(self.config, step)

    def ema_decay(self, step):
        """The EMA decay (float64) of the update that leaves global_step == step."""
        return ema_decay(step)

    # ------------------------------------------------------------------ the update
    def gradient_rows(self):
        """A copy of the update table (TENSOR_DTYPE rows in `names` order) with `grad` holding the address of every parameter's
        current .grad, 0 where it is None.  Read on the host at the time of the call: what step(), norms(), histograms() and the
        gradient exchange upload."""
        import torch
        grads = np.zeros(len(self.names), np.uint64)
        for i, (name, w) in enumerate(zip(self.names, self._w_ptrs.tolist())):
            p = self.parameters[name]
            if p.data_ptr() != w:
                raise RuntimeError("the storage of parameter %r was replaced after TrainStep was built" % name)
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or g.device != self.device or g.shape != p.shape or not g.is_contiguous() or g.data_ptr() % 4:
                raise ValueError("the gradient of %r must be a contiguous float32 tensor of the parameter's shape and device" % name)
            grads[i] = g.data_ptr()
        rows = self._table.view(np.uint8).copy().view(TENSOR_DTYPE)     # as bytes: NumPy copies a structured array field by field
        rows["grad"] = grads
        return rows

    def step(self):
        """One update from the parameters' current .grad (None: that parameter keeps its value and slots, its average still moves).
        Enqueues on the current stream and returns; global_step is incremented."""
        import torch
        if torch.cuda.is_current_stream_capturing():
            # the step's scalars are kernel arguments and the gradients' addresses are read here, on the host: a captured launch
            # would replay this step's values for ever
            raise RuntimeError("TrainStep.step() cannot be captured into a graph: the learning rate, the EMA decay and the gradient "
                               "addresses change from step to step on the host; call it outside the capture")
        rows = self.gradient_rows()
        t = self.global_step + 1
        scalars = step_scalars(self.config, t)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            host, dev = self._ring.upload(rows, stream)
            _lib.check(_lib.lib().ssd_train_update(host.data_ptr(), dev.data_ptr(), len(self.names), ctypes.byref(scalars),
                                                   stream.cuda_stream))
        self.global_step = t
        return t

    # ------------------------------------------------------------------ the norms
    def norms(self):
        """(sums, bad) of the parameters and their current .grad (include/ssd_hip.h, "the TRAIN step's norms"): sums float64 [T,2]
        holds sum w^2 and sum g^2, bad int64 [T,2] the non-finite elements of w and of the gradient, rows in `names` order; a
        parameter whose .grad is None gives 0 and 0.  Called BEFORE step(): the values are of the variables the step computed with.
        One small asynchronous upload (a TableRing of its own, made by the first call: step()'s is not touched) and two launches on
        the current stream; never waits for the device; the results are CUDA tensors of this call."""
        import torch
        from . import train_calls
        if torch.cuda.is_current_stream_capturing():
            # the gradients' addresses are read here, on the host: a captured launch would replay this step's addresses for ever
            raise RuntimeError("TrainStep.norms() cannot be captured into a graph: the gradient addresses change from step to step "
                               "on the host; call it outside the capture")
        T = len(self.names)
        rows = self.gradient_rows()
        with torch.cuda.device(self.device):
            if self._norms_ring is None:
                self._norms_ring = TableRing(self.device, TENSOR_DTYPE, T)
            sums = torch.empty((T, 2), dtype=torch.float64, device=self.device)
            bad = torch.empty((T, 2), dtype=torch.int64, device=self.device)
            host, dev = self._norms_ring.upload(rows)
            train_calls.train_norms(host, dev, sums, bad)
        return sums, bad

    # ------------------------------------------------------------------ the histograms
    def histograms(self):
        """(counts, stats) of the parameters and of the gradients of total_loss (include/ssd_hip.h, "the TRAIN step's histograms"):
        counts int64 [T,2,NB] over train_calls.histogram_limits(), stats uint8 [T,2,40] (train_calls.STATS_DTYPE on the host), plane
        0 the variable, plane 1 its current .grad plus weight_decay * w where the variable decays; rows in `names` order; a
        parameter whose .grad is None gives an all-zero plane 1 with num = 0.  Called BEFORE step(), like norms(), whose discipline
        this is: one small asynchronous upload from a TableRing of its own, made by the first call (step()'s and norms()' are not
        touched), a fixed number of launches on the current stream, never waits for the device; the results are CUDA tensors of
        this call.  The limits are uploaded once per TrainStep, by the first call."""
        import torch
        from . import train_calls
        if torch.cuda.is_current_stream_capturing():
            # the gradients' addresses are read here, on the host: a captured launch would replay this step's addresses for ever
            raise RuntimeError("TrainStep.histograms() cannot be captured into a graph: the gradient addresses change from step to "
                               "step on the host; call it outside the capture")
        T = len(self.names)
        rows = self.gradient_rows()
        with torch.cuda.device(self.device):
            if self._hist_ring is None:
                self._hist_ring = TableRing(self.device, TENSOR_DTYPE, T)
                self._hist_limits = torch.from_numpy(train_calls.histogram_limits().copy()).to(self.device)
            counts = torch.empty((T, 2, self._hist_limits.numel()), dtype=torch.int64, device=self.device)
            stats = torch.empty((T, 2, train_calls.STATS_BYTES), dtype=torch.uint8, device=self.device)
            host, dev = self._hist_ring.upload(rows)
            train_calls.train_histograms(host, dev, np.float32(self.config["weight_decay"]), self._hist_limits, counts, stats)
        return counts, stats

    def regularization_loss(self, sums_host):
        """model.py:80-81 from norms()' sums read back to the host ([T,2] float64): fp32(weight_decay * sum over the decaying rows,
        in `names` order, of sums[t,0] / 2), formed in float64 and rounded once -- evaluation.regularization_loss's definition on
        the GPU's per-tensor sums."""
        sums_host = np.asarray(sums_host, np.float64)
        if sums_host.shape != (len(self.names), 2):
            raise ValueError("sums_host must be norms()' sums, shape [%d, 2]" % len(self.names))
        s = 0.0
        for t in np.nonzero(self._table["decay"])[0]:
            s += float(sums_host[t, 0]) / 2.0
        return np.float32(float(self.config["weight_decay"]) * s)

    # ------------------------------------------------------------------ checkpoints
    def _export(self, name, tensor):
        a = tensor.detach().cpu().numpy()
        return to_tf_layout(name, a) if self.layout == "torch" else np.ascontiguousarray(a)

    def save(self, model_dir):
        """Writes model_dir/model.ckpt-<global_step>.{index,data-00000-of-00001} and the `checkpoint` state file: every parameter
        and statistic under its reference name, `<name>/ExponentialMovingAverage`, `global_step`, and the optimizer's slots
        (`optimizer/<name>/Adam`, `/Adam_1`, `optimizer/beta1_power`, `optimizer/beta2_power`).  Returns the prefix."""
        os.makedirs(model_dir, exist_ok=True)
        out = {}
        for name in self.names:
            m, v = self.slots(name)
            out[name] = self._export(name, self.parameters[name])
            out[name + EMA_SUFFIX] = self._export(name, self.ema(name))
            out["optimizer/%s/Adam" % name] = self._export(name, m)
            out["optimizer/%s/Adam_1" % name] = self._export(name, v)
        for name, s in self.statistics.items():
            out[name] = np.ascontiguousarray(s.detach().cpu().numpy())
        out.update(self.frozen)
        # TF's accumulators start at beta and are multiplied once per apply: beta^(global_step + 1)
        out["optimizer/beta1_power"] = np.float32(BETA1 ** (self.global_step + 1))
        out["optimizer/beta2_power"] = np.float32(BETA2 ** (self.global_step + 1))
        out["global_step"] = np.int64(self.global_step)
        base = "model.ckpt-%d" % self.global_step
        prefix = write_checkpoint(os.path.join(model_dir, base), out)
        write_checkpoint_state(model_dir, base)
        return prefix

    def restore(self, path):
        """The inverse of save from a model_dir, a prefix or one of its files: parameters, statistics, averages, slots and
        global_step; the next step() continues as if the run had not been interrupted."""
        import torch
        prefix = resolve_checkpoint(path)
        if prefix is None:
            raise FileNotFoundError("%s is not a checkpoint prefix or model_dir" % path)
        _, entries = read_checkpoint_index(prefix)
        want = ["global_step"] + list(self.statistics)
        for name in self.names:
            want += [name, name + EMA_SUFFIX, "optimizer/%s/Adam" % name, "optimizer/%s/Adam_1" % name]
        missing = [n for n in want if n not in entries]
        if missing:
            raise KeyError("checkpoint %s has no variable %r" % (prefix, missing[0]))
        got = read_checkpoint(prefix, want)

        def load(dst, key, name):
            a = got[key]
            if self.layout == "torch":
                a = from_tf_layout(name, a)
            if a.dtype != np.float32 or tuple(a.shape) != tuple(dst.shape):
                raise ValueError("variable %r has shape %s dtype %s, expected %s float32" % (key, a.shape, a.dtype, tuple(dst.shape)))
            with torch.no_grad():
                dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        for name in self.names:
            m, v = self.slots(name)
            load(self.parameters[name], name, name)
            load(self.ema(name), name + EMA_SUFFIX, name)
            load(m, "optimizer/%s/Adam" % name, name)
            load(v, "optimizer/%s/Adam_1" % name, name)
        for name, s in self.statistics.items():
            load(s, name, "")
        self.global_step = int(got["global_step"])
        return prefix
