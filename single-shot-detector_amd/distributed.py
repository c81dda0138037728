"""Multi-GPU: images shard over ranks (one process per GPU), detections are exchanged with
ONE all-gather of fixed-size records per batch (RCCL over xGMI with backend 'nccl'; the
same code runs on gloo/CPU tensors in the tests).  The reference has no multi-GPU code;
every image is independent end to end (nms.py:96-101 maps over images), so no other
collective exists on the path.

Record per image: ssd.split_records (6T+1 32-bit words, 48 004 B at T = 2000).
"""
import os

import torch
import torch.distributed as dist

from .ssd import host_frame, mixed_batches, pack_records, score_filter, split_records


def bind_to_gpu_numa_node(device=0):
    """One process per GPU, on the GPU's own NUMA node: restricts this process (and the threads it starts later) to the CPUs
    of the node the device hangs off (sysfs numa_node of its PCI function).  The host side of a small call -- staging memcpy
    into pinned memory, kernel launches, reading results the GPU wrote into pinned memory -- runs measurably faster there:
    batch-1 `Detector.__call__` p50 1.700 ms bound to the GPU's node, 1.743 bound to the other one, 1.71-1.75 unbound
    (scripts/numa_probe.py, profiles/r03_numa_probe.log).  Call it before creating the Detector (pinned buffers are placed by
    first touch).  Returns the node, or None when the topology is not readable (then nothing is changed)."""
    import glob
    import os
    try:
        pr = torch.cuda.get_device_properties(device)
        bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return None
        cpus = []
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            if "-" in part:
                a, b = part.split("-")
                cpus.extend(range(int(a), int(b) + 1))
            elif part:
                cpus.append(int(part))
        cpus = sorted(set(cpus) & set(os.sched_getaffinity(0)))
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return node
    except Exception:            # no GPU, no sysfs, a torch build without the PCI fields: leave the process as it is
        return None


def shard_range(total, rank, world_size):
    """Contiguous split of `total` images: rank r gets [lo, hi)."""
    base, rem = divmod(total, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def pack_detections(boxes, labels, scores, num):
    """The four outputs of a batch -> a new record block [B, 6T+1] beside them."""
    return pack_records(boxes, labels, scores, num)


def unpack_detections(rec):
    """(boxes, labels, scores, num) as VIEWS of a record block [B, 6T+1]: no copy, no launch."""
    return split_records(rec)


def gather_records(rec, group=None, out=None):
    """ONE all-gather of the [B_local, 6T+1] int32 records -> [world*B_local, 6T+1], rank order.  `out`: the receive
    buffer; when `rec` is this rank's slice of it the collective runs in place (RCCL: sendbuff == recvbuff + rank * count)."""
    world = dist.get_world_size(group)
    if out is None:
        out = torch.empty((world * rec.shape[0], rec.shape[1]), dtype=rec.dtype, device=rec.device)
    # One-buffer form everywhere (RCCL has it, and so does this image's gloo); only a backend that says it does not
    # implement it takes the list form.  Any other error is a real failure and propagates unchanged.
    try:
        dist.all_gather_into_tensor(out, rec, group=group)
    except NotImplementedError:
        parts = [torch.empty_like(rec) for _ in range(world)]
        dist.all_gather(parts, rec, group=group)
        out = torch.cat(parts, 0)
    return out


def all_gather_detections(boxes, labels, scores, num, group=None, total=None, force=False):
    """Every rank contributes the records of its B_local images and receives all records in
    rank order.  `total` = the global image count when the shards are uneven
    (shard_range(total, rank, world)): the records are padded to the largest shard for the ONE
    all-gather (fixed-size operands) and the pad rows are dropped afterwards.
    A group of one rank needs no exchange and returns its inputs; `force` runs the pack -> all-gather ->
    unpack path even then (bench.py --force-dist: the collective path through RCCL on a one-GPU box)."""
    if not (dist.is_available() and dist.is_initialized()):
        return boxes, labels, scores, num
    if dist.get_world_size(group) == 1 and not force:
        return boxes, labels, scores, num
    rec = pack_detections(boxes, labels, scores, num)

    def gather(per):
        if per == rec.shape[0]:
            return gather_records(rec, group)
        pad = torch.zeros((per, rec.shape[1]), dtype=rec.dtype, device=rec.device)
        pad[:rec.shape[0]] = rec
        return gather_records(pad, group)
    return _gather_shards(rec.shape[0], total, dist.get_world_size(group), gather)


def _gather_shards(n, total, world, gather):
    """The one all-gather of a rank's shard of n images, uneven shards included: `gather(per)` runs it with every rank's part
    `per` rows high -- n, or the largest shard ceil(total / world) when `total` (shard_range's split) does not divide evenly --
    and returns the [world * per, 6T+1] records; the pad rows beyond each rank's own shard are dropped here.  Returns the
    four views of the result."""
    even = total is None or total % world == 0
    per = n if even else -(-total // world)
    if n > per:
        raise ValueError("shard of %d images exceeds ceil(%d / %d)" % (n, total, world))
    got = gather(per)
    if even:
        return unpack_detections(got)
    g3 = got.view(world, per, -1)
    shards = [shard_range(total, r, world) for r in range(world)]
    return unpack_detections(torch.cat([g3[r, :hi - lo] for r, (lo, hi) in enumerate(shards)], 0))


_gather_buffers = {}


def detect_sharded(engine, images_local, group=None, total=None, force=False, on_forward_done=None):
    """One data-parallel step: this rank's shard through the HIP path, then the all-gather.
    images_local: uint8 CUDA tensor [B_local,H,W,3]; `total`, `force`: see all_gather_detections.
    The engine writes its records straight into this rank's slice of the all-gather's receive buffer (ssd_forward_records),
    the collective runs in place on it and the four results are views of the buffer: no pack / unpack launches, no stream
    users beside RCCL's.  Uneven shards: every rank's slice is the largest shard's size; the rows beyond a rank's own
    shard are dropped by one concatenation of row ranges.

    Lifetime of the results: on the collective path they are VIEWS of a receive buffer this module keeps per (engine,
    world, shard size) -- TWO buffers used alternately, so the results of step k stay intact during step k + 1 (the usual
    "consume the previous step while the next one runs" loop) and are overwritten by step k + 2.  Clone what must live
    longer.  Without a process group (or a group of one rank and no `force`) the results are fresh tensors.

    A failed collective propagates: after an RCCL error the communicator is aborted and a retry on the same process group
    can hang every rank, so nothing is retried here.  Whether the send buffer may sit inside the receive buffer is decided
    once from the backend's name ('nccl' = RCCL: in place; anything else: one copy of this rank's slice).

    `on_forward_done`: called (no arguments) between the engine's forward and the collective -- bench.py records an event
    there to split a step into compute and all-gather."""
    use = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force)
    if not hasattr(engine, "record_words"):                # a stand-in engine (launcher tests): the generic path
        boxes, labels, scores, num = engine.forward(images_local)
        if on_forward_done is not None:
            on_forward_done()
        return all_gather_detections(boxes, labels, scores, num, group=group, total=total, force=force)
    if not use:
        out = engine.forward(images_local)
        if on_forward_done is not None:
            on_forward_done()
        return out
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    n = images_local.shape[0]

    def gather(per):
        key = (id(engine), world, per, str(images_local.device))
        slot = _gather_buffers.get(key)
        if slot is None:
            _gather_buffers.clear()
            slot = _gather_buffers[key] = {"bufs": [torch.zeros((world, per, engine.record_words), dtype=torch.int32,
                                                                device=images_local.device) for _ in range(2)], "turn": 0}
        buf = slot["bufs"][slot["turn"]]
        slot["turn"] ^= 1
        engine.forward(images_local, records=buf[rank, :n])
        if on_forward_done is not None:
            on_forward_done()
        inplace = dist.get_backend(group) == "nccl"
        return gather_records(buf[rank] if inplace else buf[rank].clone(), group, out=buf.view(world * per, -1))
    return _gather_shards(n, total, world, gather)


# ----------------------------------------------------------------------------- mixed sizes: round-robin chunks of a stream
def node_device_and_backend(device_count=None):
    """The backend rule of every multi-process entry point: rank r of a node uses device
    LOCAL_RANK % device_count; the backend is 'nccl' (RCCL, records in device memory, the all-gather in place) only when every
    rank of the node has a device of its own (LOCAL_WORLD_SIZE <= device_count), else 'gloo' (records in pinned host memory).
    RCCL never sees two ranks on one device.  Returns (device index, backend)."""
    import os
    if device_count is None:
        device_count = torch.cuda.device_count()
    if device_count < 1:
        raise RuntimeError("no GPU: the HIP path has no CPU fallback")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    return local % device_count, ("nccl" if local_world <= device_count else "gloo")


def init_node_process_group():
    """init_process_group for a torch.distributed.run launch (RANK, WORLD_SIZE, MASTER_ADDR / MASTER_PORT in the environment)
    under node_device_and_backend's rule; makes the rank's device the current one.  Returns (device index, backend)."""
    import os
    device, backend = node_device_and_backend()
    torch.cuda.set_device(device)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if backend == "nccl":
        dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return device, backend


def launch_local(nproc, module, argv, env=None):
    """`python -m MODULE --gpus N ...` typed as is: run MODULE under torch.distributed.run with `nproc` ranks on this node as
    a CHILD process (never exec: the caller has not touched the GPU and never does) and return its exit code.  The
    repository root goes in front of PYTHONPATH so that every rank imports this package."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ if env is None else env)
    env["PYTHONPATH"] = os.pathsep.join([root] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(nproc)),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "--module", module] + list(argv)
    return subprocess.call(cmd, env=env)


def read_worker_count(read_workers=None):
    """The threads that read and decode a chunk's files: `read_workers`, by default min(16, CPUs); at least one."""
    return max(1, int(read_workers if read_workers is not None else min(16, os.cpu_count() or 1)))


class ChunkAssignment:
    """Round-robin chunks of an input stream: image i belongs to rank (i // chunk) % world.  A rank decides from the index
    alone, so no total count is needed up front (a .tfrecords stream has none).  Round k is images [k * world * chunk,
    (k + 1) * world * chunk): one chunk per rank; the last round may be ragged and a rank may have no image at all.  With
    world = 1 the chunks are exactly the one-process run's chunks of `chunk` images, so batches are composed the same way.

    The rows the ranks gather are in RANK order (all of rank 0's images, then rank 1's, ...); `input_index(counts)` gives the
    input index of every such row and `to_input_order` puts the rows back in input order."""

    def __init__(self, world, rank, chunk):
        if world < 1 or not 0 <= rank < world or chunk < 1:
            raise ValueError("need world >= 1, 0 <= rank < world, chunk >= 1 (got %r, %r, %r)" % (world, rank, chunk))
        self.world, self.rank, self.chunk = int(world), int(rank), int(chunk)

    def owner(self, i):
        return (int(i) // self.chunk) % self.world

    def mine(self, i):
        return self.owner(i) == self.rank

    def select(self, items):
        """This rank's (input index, item) pairs of an iterable, in input order (every item is visited, only this rank's are
        returned)."""
        for i, x in enumerate(items):
            if self.mine(i):
                yield i, x

    def count(self, total, rank=None):
        """Images of `rank` (default: this one) among `total`."""
        r = self.rank if rank is None else rank
        full, rest = divmod(int(total), self.world * self.chunk)
        return full * self.chunk + min(max(rest - r * self.chunk, 0), self.chunk)

    def input_index(self, counts):
        """counts[r] = images of rank r -> int64 array: the input index of every gathered row (rank order).  Raises when the
        counts are not a round-robin split of sum(counts) images."""
        import numpy as np
        if len(counts) != self.world:
            raise ValueError("need one count per rank, got %d for world %d" % (len(counts), self.world))
        parts = []
        for r, n in enumerate(counts):
            j = np.arange(int(n), dtype=np.int64)
            parts.append(((j // self.chunk) * self.world + r) * self.chunk + j % self.chunk)
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        if not np.array_equal(np.sort(idx), np.arange(len(idx))):
            raise ValueError("counts %s are not a round-robin split in chunks of %d" % (list(counts), self.chunk))
        return idx

    def to_input_order(self, rows, counts):
        """rows: a list in rank order (len = sum(counts)) -> the same rows in input order."""
        idx = self.input_index(counts)
        if len(rows) != len(idx):
            raise ValueError("%d rows for %d counted images" % (len(rows), len(idx)))
        out = [None] * len(idx)
        for row, i in zip(rows, idx.tolist()):
            out[i] = row
        return out


def _all_gather_ints(values, group, device):
    """A small all-gather of int64 vectors of equal length: [world, len(values)] as numpy."""
    world = dist.get_world_size(group)
    mine = torch.tensor(list(values), dtype=torch.int64, device=device)
    out = torch.empty((world, len(values)), dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(out.view(-1), mine, group=group)
    return out.cpu().numpy()


_mixed_buffers = {}


def detect_many_sharded(detector, images, group=None, score_threshold=0.1, max_batch=32, chunk=256):
    """Detector.detect_many over the ranks of `group`: every rank passes ITS OWN list of images (any sizes, any count,
    also none) and gets back every rank's per-image (boxes, labels, scores) in rank order -- each bit for bit what
    detect_many returns for that image (every image is independent end to end, nms.py:96-101).  Without an initialised
    process group this is detect_many itself; `group` None with one is the default group (also at world 1: the collective
    path runs).  Mode f32 only.

    Data flow (detect_sharded's design): one small all-gather of the per-rank counts and one of every rank's processing
    order; then per round of at most `chunk` images per rank, the engine writes its records (ssd_forward_mixed_host, batches
    as detect_many forms them) straight into this rank's slice of a receive buffer [world, max_local, 6T+1] and ONE
    all-gather of that buffer runs.  Records live in device memory with backend 'nccl' (the gather in place) and in pinned
    host memory otherwise (node_device_and_backend).  At most world x chunk records (48 004 B each at T = 2000) per round."""
    import numpy as np
    from .ssd import Engine
    if not (dist.is_available() and dist.is_initialized()):
        return detector.detect_many(images, score_threshold=score_threshold, max_batch=max_batch)
    eng = detector.engine
    if eng.precision != "f32":
        raise ValueError("detect_many_sharded runs in mode f32 (the precision of detect_many's batched path)")
    imgs = [host_frame(im, "every image") for im in images]
    chunk = max(1, int(chunk))
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    on_device = dist.get_backend(group) == "nccl"
    small = torch.device("cuda", eng.device) if on_device else torch.device("cpu")
    counts = _all_gather_ints([len(imgs)], group, small)[:, 0]
    # this rank's processing order: per round of `chunk` images, detect_many's batches back to back
    order, batches = [], []
    for k0 in range(0, len(imgs), chunk):
        parts = mixed_batches(eng, [im.shape[:2] for im in imgs[k0:k0 + chunk]], max_batch)
        batches.append([[k0 + i for i in p] for p in parts])
        order += [k0 + i for p in parts for i in p]
    most = int(counts.max()) if len(counts) else 0
    padded = order + [-1] * (most - len(order))
    orders = _all_gather_ints(padded, group, small) if most else np.zeros((world, 0), np.int64)
    words = eng.record_words
    rounds = -(-most // chunk)
    pinned = not on_device and torch.cuda.is_available() and isinstance(eng, Engine)   # (a stand-in engine writes on the CPU)
    need = world * min(chunk, most) * words
    key = (id(eng), eng.device, on_device)
    buf = _mixed_buffers.get(key)
    if need and (buf is None or buf.numel() < need):           # grow-only, one per engine
        _mixed_buffers.clear()
        if on_device:
            buf = torch.zeros((need,), dtype=torch.int32, device=small)
        elif pinned:
            buf = torch.zeros((need,), dtype=torch.int32).pin_memory()
        else:
            buf = torch.zeros((need,), dtype=torch.int32)
        _mixed_buffers[key] = buf
    results = [[None] * int(c) for c in counts]
    with eng.lock:
        for k in range(rounds):
            per = int(min(chunk, max(int(c) - k * chunk for c in counts)))
            got = buf[:world * per * words].view(world, per, words)
            row = 0
            for part in (batches[k] if k < len(batches) else []):
                eng.forward_mixed_host([imgs[i] for i in part], records=got[rank, row:row + len(part)])
                row += len(part)
            if pinned:
                torch.cuda.current_stream(eng.device).synchronize()      # the kernels' writes into pinned memory, before gloo reads
            gather_records(got[rank] if on_device else got[rank].clone(), group, out=got.view(world * per, words))
            host = got.cpu().numpy() if on_device else got.numpy()
            for r in range(world):
                n_r = int(min(chunk, max(int(counts[r]) - k * chunk, 0)))
                boxes, labels, scores, num = split_records(host[r, :n_r])
                for j in range(n_r):
                    results[r][int(orders[r, k * chunk + j])] = score_filter(boxes[j], labels[j], scores[j], num[j], score_threshold)
    return [x for per_rank in results for x in per_rank]
