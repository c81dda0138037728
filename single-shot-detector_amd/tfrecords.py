"""The reference's validation data without TensorFlow: `.tfrecords` shards written by data/create_tfrecords.py (one
tf.train.Example per image, :116-123: 'image' JPEG bytes, 'ymin' / 'xmin' / 'ymax' / 'xmax' float lists normalised to
[0, 1], 'labels' int64 list), read the way train.py:21-24 + pipeline.py:75-96 read them.

TFRecord framing (tensorflow/core/lib/io/record_writer.cc): uint64 length, uint32 masked CRC-32C of the length bytes,
the record, uint32 masked CRC-32C of the record; both CRCs are verified.  Example / Features / Feature / BytesList /
FloatList / Int64List are parsed from the wire format; repeated scalars are accepted packed and unpacked.
"""
import os
import struct

import numpy as np

from .ckpt_import import masked_crc32c
from .pb_import import _fields, _varint


def shard_paths(dataset_path):
    """train.py:21-24: the `.tfrecords` files of a directory in sorted order (a file path: just that file)."""
    if os.path.isfile(dataset_path):
        return [dataset_path]
    names = sorted(n for n in os.listdir(dataset_path) if n.endswith(".tfrecords"))
    return [os.path.join(dataset_path, n) for n in names]


def read_records(path, verify=True):
    """Yields the raw records of one TFRecord file (bytes)."""
    with open(path, "rb") as f:
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise ValueError("%s: truncated record header" % path)
            n, crc = struct.unpack("<QI", head)
            if verify and masked_crc32c(head[:8]) != crc:
                raise ValueError("%s: corrupt record length (CRC mismatch)" % path)
            data = f.read(n)
            tail = f.read(4)
            if len(data) < n or len(tail) < 4:
                raise ValueError("%s: truncated record" % path)
            if verify and masked_crc32c(data) != struct.unpack("<I", tail)[0]:
                raise ValueError("%s: corrupt record (CRC mismatch)" % path)
            yield data


def write_records(path, records):
    """The framing above around every bytes object of `records` (for tests and conversions)."""
    with open(path, "wb") as f:
        for r in records:
            r = bytes(r)
            head = struct.pack("<Q", len(r))
            f.write(head + struct.pack("<I", masked_crc32c(head)) + r + struct.pack("<I", masked_crc32c(r)))


def serialize_example(image, xmin, xmax, ymin, ymax, labels):
    """The tf.train.Example of one image as create_tfrecords.py:116-123 fills it: 'image' one bytes value, the four box columns
    float lists, 'labels' an int64 list -- the map entries in THAT order (a map's order on the wire is the writer's choice and no
    reader may depend on it), repeated scalars packed, an empty list as an empty FloatList / Int64List."""
    from .ckpt_export import _field_bytes, _varint

    def floats(values):
        payload = np.asarray(values, "<f4").tobytes()
        return _field_bytes(2, _field_bytes(1, payload) if payload else b"")

    def ints(values):
        payload = b"".join(bytes(_varint(int(v) & 0xFFFFFFFFFFFFFFFF)) for v in values)
        return _field_bytes(3, _field_bytes(1, payload) if payload else b"")
    entries = [("image", _field_bytes(1, _field_bytes(1, bytes(image)))), ("xmin", floats(xmin)), ("xmax", floats(xmax)),
               ("ymin", floats(ymin)), ("ymax", floats(ymax)), ("labels", ints(labels))]
    features = b"".join(bytes(_field_bytes(1, _field_bytes(1, key.encode()) + _field_bytes(2, bytes(feature)))) for key, feature in entries)
    return bytes(_field_bytes(1, features))


def _repeated(buf, kind):
    """The `value` field (1) of a BytesList / FloatList / Int64List, packed or unpacked."""
    out = []
    for fn, wt, v in _fields(buf):
        if fn != 1:
            continue
        if kind == "bytes":
            out.append(bytes(v))
        elif kind == "float":
            if wt == 2:
                out.extend(np.frombuffer(bytes(v), "<f4").tolist())
            else:
                out.append(struct.unpack("<f", struct.pack("<I", v))[0])
        else:
            if wt == 2:
                pos, b = 0, bytes(v)
                while pos < len(b):
                    x, pos = _varint(b, pos)
                    out.append(x - (1 << 64) if x >= 1 << 63 else x)
            else:
                out.append(v - (1 << 64) if v >= 1 << 63 else v)
    return out


def parse_example(buf):
    """tf.train.Example bytes -> {feature name: list of bytes | float | int}."""
    feats = {}
    for fn, _wt, features in _fields(buf):
        if fn != 1:
            continue
        for fn2, _wt2, entry in _fields(features):
            if fn2 != 1:
                continue
            key, value = None, []
            for fn3, _wt3, v in _fields(entry):
                if fn3 == 1:
                    key = bytes(v).decode()
                elif fn3 == 2:
                    for kind_no, _wt4, lst in _fields(v):
                        value = _repeated(lst, {1: "bytes", 2: "float", 3: "int64"}.get(kind_no, "bytes"))
            if key is not None:
                feats[key] = value
    return feats


def read_example(buf):
    """One record of create_tfrecords.py -> (JPEG bytes, boxes float32 [n,4] ymin,xmin,ymax,xmax, labels int32 [n])
    (pipeline.py:75-96: the box columns stacked in that order, labels cast to int32)."""
    f = parse_example(buf)
    cols = [np.asarray(f.get(k, []), np.float32) for k in ("ymin", "xmin", "ymax", "xmax")]
    if len({c.size for c in cols}) != 1 or len(f.get("labels", [])) != cols[0].size:
        raise ValueError("example: box columns and labels differ in length")
    image = f.get("image", [])
    if len(image) != 1:
        raise ValueError("example: expected one 'image'")
    return image[0], np.stack(cols, axis=1).reshape(-1, 4), np.asarray(f["labels"], np.int64).astype(np.int32)


def read_dataset(dataset_path, verify=True):
    """Yields (JPEG bytes, boxes, labels) over every shard of `dataset_path` in train.py's order."""
    for path in shard_paths(dataset_path):
        for r in read_records(path, verify=verify):
            yield read_example(r)


def decode_image(x):
    """The decode of the pipelines (tf.image.decode_jpeg(channels=3)): JPEG bytes -> uint8 [H, W, 3] through PIL; an array
    passes through."""
    if isinstance(x, np.ndarray):
        return x
    import io
    from PIL import Image
    with Image.open(io.BytesIO(x)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)
