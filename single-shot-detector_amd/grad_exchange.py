"""Data-parallel training's one collective per step (include/ssd_hip.h, "the TRAIN step's gradient exchange"):
every rank packs its gradients, its moving statistics and a 3-word header (matches, localization loss, classification loss) into
its slice of a receive buffer, ONE all-gather moves the slices, and one kernel sums them in ascending rank order back into the
gradients and the statistics.  Every rank computes the same bits from the same bytes, whatever the backend: over 'nccl' (RCCL) the
slice is written in place into the device receive buffer; over any other backend it goes through pinned host memory
(distributed.node_device_and_backend's rule).  A group of one rank is the identity, bit for bit.
"""
import hashlib

import numpy as np

from . import train_calls
from .train_step import TableRing


def agree_on_table(table, group, device):
    """The check that every rank exchanges the same table (train_calls.REDUCE_ROW_DTYPE rows): ONE fixed-size all-gather of a
    digest of (T, counts, kinds, which gradients are present) over tensors on `device`, so no rank waits for another; a mismatch
    raises ValueError on every rank."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    h = hashlib.sha256()
    h.update(np.int64(len(table)).tobytes())
    h.update(np.ascontiguousarray(table["count"]).tobytes())
    h.update(np.ascontiguousarray(table["kind"]).tobytes())
    h.update((table["data"] != 0).astype(np.uint8).tobytes())
    mine = torch.from_numpy(np.frombuffer(h.digest(), np.uint8).view(np.int64).copy()).to(device)
    got = torch.empty((world, mine.numel()), dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(got.view(-1), mine, group=group)
    got = got.cpu().numpy()
    differ = [r for r in range(world) if not np.array_equal(got[r], got[0])]
    if differ:
        raise ValueError("the ranks do not exchange the same tensors: rank(s) %s differ from rank 0 in the number of rows, their "
                         "counts or kinds, or in which gradients are present" % differ)


class GradientExchange:
    """The exchange of one TrainStep's gradients over the ranks of `group`.

    train_step   the TrainStep whose parameters' current .grad are exchanged (rows of kind 0, in `names` order; a parameter whose
                 .grad is None ships zeros and receives nothing)
    statistics   {name: float32 CUDA tensor}: the moving means and variances, averaged over the ranks with weight 1 / G (rows of
                 kind 1, in the dict's order); may be empty
    group        a torch.distributed process group (None: the default group), 1 .. 16 ranks

    exchange(header) -> (localization_loss, classification_loss, weights): the two losses over the global batch as device scalars
    and the ranks' weights c_r [G]; afterwards every .grad and every statistic holds the reduced value.  One small asynchronous
    upload from a train_step.TableRing of its own, two launches and one all-gather on the current stream; over 'nccl' it never waits
    for the device.  Two receive buffers are used alternately."""

    def __init__(self, train_step, statistics, group=None):
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("GradientExchange needs an initialised torch.distributed process group")
        self.train_step = train_step
        self.group = group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        if not 1 <= self.world <= train_calls.REDUCE_MAX_RANKS:
            raise ValueError("the group has %d ranks, the exchange takes 1 .. %d" % (self.world, train_calls.REDUCE_MAX_RANKS))
        self.on_device = dist.get_backend(group) == "nccl"
        self.device = train_step.device
        self.statistics = dict(statistics or {})
        for name, s in self.statistics.items():
            if not (isinstance(s, torch.Tensor) and s.dtype == torch.float32 and s.device == self.device and s.is_contiguous()
                    and s.data_ptr() % 4 == 0):
                raise ValueError("statistic %r must be a contiguous float32 tensor on %s" % (name, self.device))
        params = [train_step.parameters[n] for n in train_step.names]
        self.T = len(params) + len(self.statistics)
        table = np.zeros(self.T, train_calls.REDUCE_ROW_DTYPE)
        table["count"] = [p.numel() for p in params] + [s.numel() for s in self.statistics.values()]
        table["kind"] = [0] * len(params) + [1] * len(self.statistics)
        table["offset"], self.slice_floats = train_calls.bucket_layout(table["count"])
        table["data"][len(params):] = [s.data_ptr() for s in self.statistics.values()]
        self._table = table
        self._ring = TableRing(self.device, train_calls.REDUCE_ROW_DTYPE, self.T)
        with torch.cuda.device(self.device):
            self._bufs = [torch.zeros((self.world, self.slice_floats), dtype=torch.float32, device=self.device) for _ in range(2)]
            if not self.on_device:
                self._send = torch.zeros(self.slice_floats, dtype=torch.float32).pin_memory()
                self._recv = [torch.zeros((self.world, self.slice_floats), dtype=torch.float32).pin_memory() for _ in range(2)]
        self._turn = 0
        self._agreed = False

    def _rows(self):
        """This call's table: the gradients' addresses as they are now (TrainStep.gradient_rows, with its checks)."""
        table = self._table.copy()
        grads = self.train_step.gradient_rows()["grad"]
        table["data"][:len(grads)] = grads
        return table

    def exchange(self, header):
        import torch
        import torch.distributed as dist
        if torch.cuda.is_current_stream_capturing():
            # the gradients' addresses are read here, on the host: a captured launch would replay this step's addresses for ever
            raise RuntimeError("GradientExchange.exchange() cannot be captured into a graph: the gradient addresses change from step "
                               "to step on the host; call it outside the capture")
        if not (isinstance(header, torch.Tensor) and header.dtype == torch.float32 and header.device == self.device
                and tuple(header.shape) == (3,) and header.is_contiguous()):
            raise ValueError("header must be a contiguous float32 tensor [3] (matches, localization loss, classification loss) on %s"
                             % self.device)
        table = self._rows()
        if not self._agreed:
            agree_on_table(table, self.group, self.device if self.on_device else torch.device("cpu"))
            self._agreed = True
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rows_host, rows_dev = self._ring.upload(table, stream)
            buf = self._bufs[self._turn]
            train_calls.train_grad_pack(rows_host, rows_dev, header, buf[self.rank])
            if self.on_device:
                dist.all_gather_into_tensor(buf.view(-1), buf[self.rank], group=self.group)      # in place (RCCL)
            else:
                recv = self._recv[self._turn]
                self._send.copy_(buf[self.rank], non_blocking=True)
                stream.synchronize()                 # the slice is in pinned memory (and the previous upload of `recv` has run)
                dist.all_gather_into_tensor(recv.view(-1), self._send, group=self.group)
                buf.copy_(recv, non_blocking=True)
            losses = torch.empty(2, dtype=torch.float32, device=self.device)
            weights = torch.empty(self.world, dtype=torch.float32, device=self.device)
            train_calls.train_grad_reduce(rows_host, rows_dev, buf, losses, weights)
        self._turn ^= 1
        return losses[0], losses[1], weights
