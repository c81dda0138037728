"""Writes a TensorFlow V2 checkpoint ("tensor bundle") without TensorFlow: the inverse of ckpt_import.py.

`write_checkpoint(prefix, tensors)` leaves `prefix.index` and `prefix.data-00000-of-00001`, `write_checkpoint_state` the
`checkpoint` state file of a model_dir (what tf.train.latest_checkpoint and ckpt_import.resolve_checkpoint read).  The format is
the one the module docstring of ckpt_import.py describes, from the writing side:

  * the data shard holds every tensor's little-endian bytes back to back, in key order;
  * the index is a LevelDB-format table: data blocks of prefix-compressed entries (shared / unshared / value lengths as varint32,
    a restart point -- an entry with shared = 0 -- every 16 entries, the restart offsets and their count as uint32 at the block's
    end), each followed by a compression byte (0) and the masked CRC-32C of block + byte; an empty metaindex block; an index
    block whose keys are each data block's last key (a valid separator: >= every key of the block, < every key of the next) and
    whose values are the block handles (varint offset, varint size), one restart per entry; a 48-byte footer (the two handles,
    zero padding, the magic);
  * key "" holds BundleHeaderProto {num_shards = 1, version {producer = 1}}, every other key a BundleEntryProto {dtype, shape,
    offset, size, crc32c (masked, fixed32)}; proto3 encoding by hand, zero-valued scalar fields left out as protobuf does.

The checksum is ckpt_import's (one CRC-32C in the package); nothing here depends on google.protobuf.  The tests read the result
back with ckpt_import.read_checkpoint(verify=True); no TensorFlow is reachable to read it with, so acceptance by TensorFlow's own
BundleReader is unverified.
"""
import os
import struct

import numpy as np

from .ckpt_import import TABLE_MAGIC, FOOTER_BYTES, masked_crc32c

BLOCK_BYTES = 262144            # table::Options::block_size of TensorFlow's table builder
RESTART_INTERVAL = 16
# numpy -> types.proto DataType (the inverse of ckpt_import._DTYPES for what a training run stores)
_DTYPE_NUMBERS = {np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.int32): 3, np.dtype(np.int64): 9}


def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _field_varint(number, v):
    return _varint(number << 3) + _varint(v) if v else b""


def _field_bytes(number, payload):
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def _shape_proto(shape):
    # TensorShapeProto: repeated Dim dim = 2 {int64 size = 1}
    return b"".join(_field_bytes(2, _field_varint(1, int(d))) for d in shape)


def _entry_proto(dtype_number, shape, offset, size, crc):
    # BundleEntryProto: dtype = 1, shape = 2, shard_id = 3 (0: left out), offset = 4, size = 5, crc32c = 6 (fixed32)
    return (_field_varint(1, dtype_number) + _field_bytes(2, _shape_proto(shape)) + _field_varint(4, offset) +
            _field_varint(5, size) + _varint(6 << 3 | 5) + struct.pack("<I", crc))


def _header_proto():
    # BundleHeaderProto: num_shards = 1, endianness = 2 (LITTLE = 0: left out), version = 3 {producer = 1}
    return _field_varint(1, 1) + _field_bytes(3, _field_varint(1, 1))


class _BlockBuilder:
    def __init__(self, restart_interval):
        self.interval = restart_interval
        self.buf = bytearray()
        self.restarts = [0]
        self.count = 0
        self.last = b""

    def add(self, key, value):
        shared = 0
        if self.count and self.count % self.interval == 0:
            self.restarts.append(len(self.buf))
        elif self.count:
            n = min(len(key), len(self.last))
            while shared < n and key[shared] == self.last[shared]:
                shared += 1
        self.buf += _varint(shared) + _varint(len(key) - shared) + _varint(len(value)) + key[shared:] + value
        self.last = key
        self.count += 1

    def size(self):
        return len(self.buf) + 4 * len(self.restarts) + 4

    def finish(self):
        return bytes(self.buf) + b"".join(struct.pack("<I", r) for r in self.restarts) + struct.pack("<I", len(self.restarts))


def write_table(path, items, block_bytes=BLOCK_BYTES):
    """A LevelDB-format table file of `items` ((key bytes, value bytes), any order; keys unique).  block_bytes: a data block is
    closed once it holds at least that many bytes."""
    items = sorted(items)
    for (a, _), (b, _) in zip(items, items[1:]):
        if a == b:
            raise ValueError("duplicate table key %r" % a)
    out = bytearray()

    def emit(block):
        handle = _varint(len(out)) + _varint(len(block))
        out.extend(block)
        out.append(0)                                                        # kNoCompression
        out.extend(struct.pack("<I", masked_crc32c(block + b"\0")))
        return handle

    index = _BlockBuilder(1)
    cur = _BlockBuilder(RESTART_INTERVAL)
    for key, value in items:
        cur.add(key, value)
        if cur.size() >= block_bytes:
            index.add(cur.last, emit(cur.finish()))
            cur = _BlockBuilder(RESTART_INTERVAL)
    if cur.count or not index.count:
        index.add(cur.last, emit(cur.finish()))
    meta = emit(_BlockBuilder(RESTART_INTERVAL).finish())
    foot = meta + emit(index.finish())
    out.extend(foot + b"\0" * (FOOTER_BYTES - 8 - len(foot)) + struct.pack("<Q", TABLE_MAGIC))
    with open(path, "wb") as f:
        f.write(out)


def write_checkpoint(prefix, tensors, block_bytes=BLOCK_BYTES):
    """Writes {name: ndarray} (float32, float64, int32 or int64; any shape, scalars included) as the bundle `prefix`.  Both files
    are written beside their final names and renamed, the index last: a reader never sees an index without its data."""
    names = sorted(tensors, key=lambda n: n.encode())
    if "" in tensors:
        raise ValueError('the key "" is the bundle header')
    data_path = "%s.data-00000-of-00001" % prefix
    items = [(b"", _header_proto())]
    offset = 0
    with open(data_path + ".tmp", "wb") as f:
        for name in names:
            a = np.asarray(tensors[name])
            number = _DTYPE_NUMBERS.get(a.dtype.newbyteorder("="))
            if number is None:
                raise ValueError("variable %r: dtype %s is not written" % (name, a.dtype))
            raw = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<")).tobytes()
            items.append((name.encode(), _entry_proto(number, a.shape, offset, len(raw), masked_crc32c(raw))))
            f.write(raw)
            offset += len(raw)
    write_table(prefix + ".index.tmp", items, block_bytes)
    os.replace(data_path + ".tmp", data_path)
    os.replace(prefix + ".index.tmp", prefix + ".index")
    return prefix


def write_checkpoint_state(model_dir, basename):
    """The `checkpoint` state file of model_dir naming the bundle `basename` (a path relative to model_dir, as the Saver writes)."""
    tmp = os.path.join(model_dir, "checkpoint.tmp")
    with open(tmp, "w") as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (basename, basename))
    os.replace(tmp, os.path.join(model_dir, "checkpoint"))
