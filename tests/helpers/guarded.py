"""One arena per entry-point call: every tensor of the call (inputs, outputs, per-channel vectors, the workspace) inside ONE uint8
allocation, each between at least GUARD bytes of the update test's sentinel word, at bases that are 16-byte (or 4-byte) aligned and
no more.  A store past a tensor's end changes a guard word of the same allocation, which check() reports; it never leaves memory the
process owns.  Separate is the control with the same interface: every tensor its own allocation, as the other tests do.

Layouts (include/ssd_hip.h promises 16 bytes for x, dy, out, w_dev, dw_dev and the workspace, 4 for bias_dev, dbias_dev, uint8
frames and the loss's logits):
  aligned   every base = 0 (mod 512)
  skewed    the i-th tensor of contract 16 at base = 16 * o (mod 256), o = 1, 3, .., 15 in turn: never a multiple of 32;
            the j-th tensor of contract 4 at base = 4, 8, 12 (mod 16) in turn
  mixed     the first input at 0 (mod 512), every other tensor as in skewed
The guard behind a tensor starts at its last byte + 1; every byte between two tensors is a guard byte."""
import numpy as np

GUARD = 1024                                   # the widest single wave store: 16 B x 64 lanes
SENTINEL = np.uint32(0x7FC0DEAD)               # tests/test_gpu_train_update.py's guard word: a NaN
LAYOUTS = ("aligned", "skewed", "mixed")
ROLES = ("input", "output", "workspace")
NAN_BITS = np.uint32(0x7FC00000)               # what an output of 4-byte elements holds before the call
_SENTINEL_BYTES = np.frombuffer(SENTINEL.tobytes(), np.uint8)


class GuardError(AssertionError):
    """check() failed: .name the tensor, .side 'front' | 'back' | 'inside', .offset in bytes -- back: from the tensor's last byte
    (1 = the first byte behind it); front: from its first byte (1 = the byte before it); inside (an input): from its first byte.
    .from_end: the first changed byte's signed distance from the tensor's last byte on every side (positive: behind the tensor)."""

    def __init__(self, name, side, offset, count, from_end):
        self.name, self.side, self.offset, self.from_end = name, side, offset, from_end
        where = {"back": "%d bytes behind the end of" % offset, "front": "%d bytes in front of" % offset,
                 "inside": "at byte %d of the input" % offset}[side]
        super().__init__("%d bytes changed that the call must not write, the first %s '%s' (%+d bytes from its last byte)"
                         % (count, where, name, from_end))


class _Tensor:
    def __init__(self, name, shape, dtype, contract, role, init):
        self.name, self.shape, self.dtype, self.contract, self.role, self.init = name, shape, dtype, contract, role, init
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        self.start = None


def _spec(name, array_or_shape, dtype, contract, role, fill, known):
    """-> _Tensor with its initial bytes: the array of an input, NaN / `fill` (a scalar or an array) for an output, 0xFF bytes for a
    workspace."""
    dtype = np.dtype(dtype)
    if role not in ROLES or contract not in (16, 4) or name in known:
        raise ValueError("add(%r): role one of %s, contract 16 or 4, a name used once" % (name, ROLES))
    if isinstance(array_or_shape, np.ndarray):
        if role != "input" or array_or_shape.dtype != dtype:
            raise ValueError("add(%r): an array of dtype %s is an input's content; outputs take fill=" % (name, dtype))
        shape, init = array_or_shape.shape, np.ascontiguousarray(array_or_shape)
    else:
        shape = tuple(int(v) for v in (array_or_shape if isinstance(array_or_shape, (tuple, list)) else (array_or_shape,)))
        if role == "input":
            raise ValueError("add(%r): an input needs its array" % name)
        if role == "workspace":
            if dtype != np.uint8 or fill is not None:
                raise ValueError("add(%r): a workspace is uint8 bytes, pre-filled with 0xFF" % name)
            init = np.full(shape, 0xFF, np.uint8)
        elif fill is None:
            if dtype.itemsize != 4:
                raise ValueError("add(%r): outputs of %s need fill=" % (name, dtype))
            init = np.full(shape, NAN_BITS, np.uint32).view(dtype)
        else:
            init = np.ascontiguousarray(np.broadcast_to(np.asarray(fill, dtype), shape))
    return _Tensor(name, tuple(shape), dtype, contract, role, init.reshape(-1).view(np.uint8))


def _torch_dtype(torch, dtype):
    return {"float32": torch.float32, "int32": torch.int32, "uint8": torch.uint8}[np.dtype(dtype).name]


class _Memory:
    """What Arena and Separate share: add() before the first view(), outputs() after the call."""

    def __init__(self, torch, device):
        self.torch, self.device, self.tensors, self.built = torch, device, {}, False

    def add(self, name, array_or_shape, dtype, contract, role, fill=None):
        if self.built:
            raise RuntimeError("add(%r) after the first view(): the layout is fixed" % name)
        self.tensors[name] = _spec(name, array_or_shape, dtype, contract, role, fill, self.tensors)
        return name

    def ptr(self, name):
        """The tensor's address for a raw ctypes call; None for name None."""
        return None if name is None else self.view(name).data_ptr()

    def outputs(self):
        """{name: numpy array} of every tensor of role output, read back from the device."""
        return {t.name: self.read(t.name) for t in self.tensors.values() if t.role == "output"}


class Separate(_Memory):
    """The control: every tensor its own allocation (512-byte aligned, rounded up by the allocator)."""

    def view(self, name):
        if name is None:
            return None
        if not self.built:
            self.built, self._dev = True, {}
            for t in self.tensors.values():
                flat = self.torch.from_numpy(t.init.copy()).to(self.device)
                self._dev[t.name] = flat.view(_torch_dtype(self.torch, t.dtype)).view(t.shape) if t.nbytes else \
                    self.torch.empty(t.shape, dtype=_torch_dtype(self.torch, t.dtype), device=self.device)
        return self._dev[name]

    def read(self, name):
        return self.view(name).cpu().numpy().copy()

    def check(self):
        for t in self.tensors.values():
            if t.role == "input" and not np.array_equal(self.read(t.name).reshape(-1).view(np.uint8), t.init):
                raise AssertionError("the input '%s' was written" % t.name)


class Arena(_Memory):
    def __init__(self, torch, device, layout="aligned"):
        super().__init__(torch, device)
        if layout not in LAYOUTS:
            raise ValueError("layout: one of %s" % (LAYOUTS,))
        self.layout = layout

    # ------------------------------------------------------------------------- the layout
    def _place(self):
        """Byte offsets of every tensor from the 512-byte aligned base -> the arena's size."""
        cursor, n16, n4, first_input = 0, 0, 0, True
        for t in self.tensors.values():
            if self.layout == "aligned" or (self.layout == "mixed" and t.role == "input" and first_input):
                modulus, residue = 512, 0
            elif t.contract == 16:
                modulus, residue = 256, 16 * (1, 3, 5, 7, 9, 11, 13, 15)[n16 % 8]
                n16 += 1
            else:
                modulus, residue = 16, (4, 8, 12)[n4 % 3]
                n4 += 1
            if t.role == "input":
                first_input = False
            least = cursor + GUARD
            t.start = least + (residue - least) % modulus
            cursor = t.start + t.nbytes + GUARD           # the guard behind starts at the last byte + 1
        return (cursor + 511) // 512 * 512 + 512          # no tensor's guard ends the allocation

    def _build(self):
        self.built = True
        total = self._place()
        host = np.resize(_SENTINEL_BYTES, total)          # the sentinel WORD at every 4-byte offset of the arena
        self.mask = np.ones(total, bool)                  # True: a byte the call must leave alone
        for t in self.tensors.values():
            host[t.start:t.start + t.nbytes] = t.init
            if t.role != "input":
                self.mask[t.start:t.start + t.nbytes] = False
        self.host = host
        slack = 0 if str(self.device).startswith("cuda") else 512       # a host allocation is aligned by hand
        raw = self.torch.empty(total + slack, dtype=self.torch.uint8, device=self.device)
        self.raw = raw
        self.dev = raw[(-raw.data_ptr()) % 512 if slack else 0:][:total]
        assert self.dev.data_ptr() % 512 == 0, "the arena's base must be 512-byte aligned"
        self.dev.copy_(self.torch.from_numpy(host))

    def offset(self, name):
        """The tensor's byte offset from the arena's 512-byte aligned base."""
        if not self.built:
            self._build()
        return self.tensors[name].start

    def view(self, name):
        """The contiguous torch view of the tensor; None for name None."""
        if name is None:
            return None
        if not self.built:
            self._build()
        t = self.tensors[name]
        v = self.dev[t.start:t.start + t.nbytes].view(_torch_dtype(self.torch, t.dtype)).view(t.shape)
        assert v.is_contiguous() and v.data_ptr() == self.dev.data_ptr() + t.start and v.data_ptr() % t.contract == 0
        return v

    def read(self, name):
        return self.view(name).cpu().numpy().copy()

    # ------------------------------------------------------------------------- after the call
    def check(self):
        """ONE copy of the arena back: every guard byte still holds the sentinel and every input its bits, else GuardError."""
        if not self.built:
            self._build()
        got = self.dev.cpu().numpy()
        bad = np.nonzero((got != self.host) & self.mask)[0]
        if not len(bad):
            return
        p = int(bad[0])
        order = sorted(self.tensors.values(), key=lambda t: t.start)
        for t in order:                                   # ascending: p lies behind every earlier tensor's own guard
            end = t.start + t.nbytes
            if p < t.start:                               # whatever lies between that guard and the tensor is its front guard
                raise GuardError(t.name, "front", t.start - p, len(bad), p - (end - 1))
            if p < end:
                raise GuardError(t.name, "inside", p - t.start, len(bad), p - (end - 1))
            if p < end + GUARD:                           # the GUARD bytes behind a tensor are its own
                raise GuardError(t.name, "back", p - (end - 1), len(bad), p - (end - 1))
        raise GuardError(order[-1].name, "back", p - (end - 1), len(bad), p - (end - 1))
