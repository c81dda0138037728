"""tf.train.Example (tensorflow/core/example/{example,feature}.proto of TF r1.12: field numbers only), declared at test time
with google.protobuf's descriptor API and serialised by the official encoder, plus the TFRecord shards
data/create_tfrecords.py writes (:116-123).  `unpacked=True` declares the repeated scalars `[packed = false]`, the form
old writers emit.  Test infrastructure only."""
import io

import numpy as np
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

F = descriptor_pb2.FieldDescriptorProto


def _field(msg, name, number, ftype, label=F.LABEL_OPTIONAL, type_name=None, packed=None, oneof=None):
    f = msg.field.add()
    f.name, f.number, f.type, f.label = name, number, ftype, label
    if type_name:
        f.type_name = type_name
    if packed is not None:
        f.options.packed = packed
    if oneof is not None:
        f.oneof_index = oneof
    return f


def build(unpacked=False):
    pkg = "tfex_u" if unpacked else "tfex"
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name, fd.package, fd.syntax = pkg + "/example.proto", pkg, "proto3"
    P = "." + pkg + "."
    pk = False if unpacked else None
    for name, ftype in (("BytesList", F.TYPE_BYTES), ("FloatList", F.TYPE_FLOAT), ("Int64List", F.TYPE_INT64)):
        m = fd.message_type.add()
        m.name = name
        _field(m, "value", 1, ftype, F.LABEL_REPEATED, packed=None if ftype == F.TYPE_BYTES else pk)
    feat = fd.message_type.add()
    feat.name = "Feature"
    feat.oneof_decl.add().name = "kind"
    _field(feat, "bytes_list", 1, F.TYPE_MESSAGE, type_name=P + "BytesList", oneof=0)
    _field(feat, "float_list", 2, F.TYPE_MESSAGE, type_name=P + "FloatList", oneof=0)
    _field(feat, "int64_list", 3, F.TYPE_MESSAGE, type_name=P + "Int64List", oneof=0)
    feats = fd.message_type.add()
    feats.name = "Features"
    entry = feats.nested_type.add()
    entry.name = "FeatureEntry"
    entry.options.map_entry = True
    _field(entry, "key", 1, F.TYPE_STRING)
    _field(entry, "value", 2, F.TYPE_MESSAGE, type_name=P + "Feature")
    _field(feats, "feature", 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "Features.FeatureEntry")
    ex = fd.message_type.add()
    ex.name = "Example"
    _field(ex, "features", 1, F.TYPE_MESSAGE, type_name=P + "Features")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return {n: message_factory.GetMessageClass(pool.FindMessageTypeByName(pkg + "." + n)) for n in ("Example",)}


def example_bytes(jpeg, boxes, labels, unpacked=False):
    """create_tfrecords.py:116-123: one image's Example."""
    M = build(unpacked)
    e = M["Example"]()
    f = e.features.feature
    f["image"].bytes_list.value.append(jpeg)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    for k, name in enumerate(("ymin", "xmin", "ymax", "xmax")):
        f[name].float_list.value.extend(boxes[:, k].tolist())
    f["labels"].int64_list.value.extend(int(v) for v in labels)
    return e.SerializeToString()


def jpeg(image, quality=90):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()
