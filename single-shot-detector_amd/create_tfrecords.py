"""python -m ssd_amd.create_tfrecords --image_dir images/ --annotations_dir annotations/ --output shards/ --labels labels.txt \\
        --num_shards 100 [--seed 0] [--jpeg_device 0]

The reference's data/create_tfrecords.py without TensorFlow: `.tfrecords` shards of one tf.train.Example per image from a folder
of JPEGs and a folder of per-image JSON annotations (`python -m ssd_amd.prepare_coco` writes those).  Its five flags, and two more:
--seed makes the shuffle repeatable, --jpeg_device N re-encodes grayscale files on GPU N.

What is kept from the reference: a label's integer is its LINE INDEX in the labels file (blank lines count, and get no label);
the annotation files are shuffled (random.Random(seed); no seed: an unseeded shuffle), shard_size = ceil(files / num_shards)
counts every annotation file while a shard fills with WRITTEN examples only, the files are shard-%04d.tfrecords; an image whose
mode is neither L nor RGB, or whose format is not JPEG, is skipped and counted; a grayscale (mode L) image is re-encoded as an
RGB JPEG by PIL's default save and stored so; the output directory is replaced.  Its assertions are ValueErrors that name the
file.  What differs: the listing is sorted before the shuffle (so that a seed gives one order on every file system), an Example's
map entries are written in one fixed order (tfrecords.serialize_example), and the output directory is refused when replacing it
would delete the inputs.

The grayscale route.  Default: PIL decodes and PIL encodes, as the reference.  --jpeg_device N: jpeg.JpegDecoder turns the files
into RGB frames on the GPU (a file it refuses is read with PIL and uploaded) and jpeg.JpegEncoder encodes them there, a group of
files at a time; only the Huffman stages run on the host.  Both routes store the same bytes (include/ssd_hip.h, blocks "the JPEG
decoder" and "the JPEG encoder": each is its PIL counterpart bit for bit)."""
import argparse
import io
import itertools
import json
import math
import os
import random
import shutil

import numpy as np

from . import tfrecords

GROUP = 256                     # annotation files read ahead, so that their grayscale images are one GPU batch


def read_labels(path):
    with open(path) as f:
        labels = {line.strip(): i for i, line in enumerate(f.readlines()) if line.strip()}
    if not labels:
        raise ValueError("%s: no label" % path)
    return labels


def pil_rgb_jpeg(array):
    """The reference's to_jpeg_bytes: PIL's default save of an RGB array."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format="jpeg")
    return buf.getvalue()


class _Pending:
    """An image between reading and writing: its bytes (`gray`: still the grayscale file's) and its Example's lists."""
    __slots__ = ("path", "blob", "gray", "columns", "labels")


def read_example(annotation_path, image_dir, labels):
    """-> _Pending, or None for an image the reference skips.  ValueError, naming the file, where the reference asserts."""
    from PIL import Image
    with open(annotation_path) as f:
        annotation = json.load(f)
    name = annotation["filename"]
    if not (name.endswith(".jpg") or name.endswith(".jpeg")):
        raise ValueError("%s: the image's name must end in .jpg or .jpeg, not %r" % (annotation_path, name))
    p = _Pending()
    p.path = os.path.join(image_dir, name)
    with open(p.path, "rb") as f:
        p.blob = f.read()
    with Image.open(io.BytesIO(p.blob)) as image:
        mode, fmt, size = image.mode, image.format, image.size
    p.gray = mode == "L"
    if not p.gray and (mode != "RGB" or fmt != "JPEG"):
        return None             # (a grayscale image of any format is re-encoded, and is a JPEG then)
    width, height = int(annotation["size"]["width"]), int(annotation["size"]["height"])
    if not (width > 1 and height > 1):
        raise ValueError("%s: width and height must be above 1, not %d x %d" % (annotation_path, width, height))
    if size != (width, height):
        raise ValueError("%s: the annotation says %d x %d, %s is %d x %d" % (annotation_path, width, height, p.path, size[0], size[1]))
    ymin, xmin, ymax, xmax, p.labels = [], [], [], [], []
    for obj in annotation["object"]:
        box = obj["bndbox"]
        a, b = float(box["ymin"]) / height, float(box["xmin"]) / width
        c, d = float(box["ymax"]) / height, float(box["xmax"]) / width
        if not (a < c and b < d):
            raise ValueError("%s: a box with ymin >= ymax or xmin >= xmax: %r" % (annotation_path, box))
        if not all(0.0 <= t <= 1.0 for t in (a, b, c, d)):
            raise ValueError("%s: a box outside the image: %r" % (annotation_path, box))
        if obj["name"] not in labels:
            raise ValueError("%s: the name %r is not in the labels file" % (annotation_path, obj["name"]))
        ymin.append(a), xmin.append(b), ymax.append(c), xmax.append(d)
        p.labels.append(labels[obj["name"]])
    p.columns = (xmin, xmax, ymin, ymax)
    return p


def _gray_array(blob):
    """The reference's own read of a grayscale file: [H, W] stacked three times."""
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as image:
        y = np.array(image)
    return np.stack(3 * [y], axis=2)


class GrayRoute:
    """Grayscale files -> the RGB JPEGs the reference stores: `device` None with PIL, else on that GPU."""

    def __init__(self, device=None, pool=None):
        self.device, self.pool = device, pool
        if device is not None:
            from .jpeg import JpegDecoder, JpegEncoder
            self.dec, self.enc = JpegDecoder(device), JpegEncoder(device)

    def encode(self, blobs):
        if self.device is None:
            return [pil_rgb_jpeg(_gray_array(b)) for b in blobs]
        if not blobs:
            return []
        out = [None] * len(blobs)
        frames, refused = self.dec.decode_many(blobs, self.pool)
        taken = [i for i in range(len(blobs)) if i not in refused]
        for i, blob in zip(taken, self.enc.encode_many(frames, pool=self.pool)):
            out[i] = blob
        rest = sorted(refused)
        for i, blob in zip(rest, self.enc.encode_many([_gray_array(blobs[i]) for i in rest], pool=self.pool) if rest else []):
            out[i] = blob
        return out


def records(annotation_paths, image_dir, labels, route, counts):
    """Yields the serialised Examples in order; counts["skipped"] counts the images left out."""
    for at in range(0, len(annotation_paths), GROUP):
        group = [read_example(p, image_dir, labels) for p in annotation_paths[at:at + GROUP]]
        counts["skipped"] += sum(g is None for g in group)
        group = [g for g in group if g is not None]
        gray = [g for g in group if g.gray]
        for g, blob in zip(gray, route.encode([g.blob for g in gray])):
            g.blob = blob
        for g in group:
            yield tfrecords.serialize_example(g.blob, *g.columns, g.labels)


def _refuse_output(output, inputs):
    out = os.path.realpath(output)
    for name, path in inputs:
        real = os.path.realpath(path)
        if os.path.commonpath([out, real]) == out:
            raise ValueError("--output %s is replaced: it must not be %s (%s) or a directory above it" % (output, name, path))


def create(image_dir, annotations_dir, output, labels, num_shards=1, seed=None, jpeg_device=None, pool=None):
    """-> {"examples": annotation files, "written": Examples, "skipped": images, "shards": files, "shard_size": the size}."""
    if num_shards < 1:
        raise ValueError("num_shards must be at least 1")
    encoder = read_labels(labels)
    _refuse_output(output, (("--image_dir", image_dir), ("--annotations_dir", annotations_dir), ("--labels", labels)))
    names = sorted(os.listdir(annotations_dir))
    random.Random(seed).shuffle(names)
    shard_size = math.ceil(len(names) / num_shards)
    route = GrayRoute(jpeg_device, pool)
    shutil.rmtree(output, ignore_errors=True)
    os.mkdir(output)
    counts = {"examples": len(names), "written": 0, "skipped": 0, "shards": 0, "shard_size": shard_size}

    def counted(it):
        for r in it:
            counts["written"] += 1
            yield r
    stream = counted(records([os.path.join(annotations_dir, n) for n in names], image_dir, encoder, route, counts))
    for first in stream:
        path = os.path.join(output, "shard-%04d.tfrecords" % counts["shards"])
        tfrecords.write_records(path, itertools.chain([first], itertools.islice(stream, shard_size - 1)))
        counts["shards"] += 1
    return counts


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    p.add_argument("-i", "--image_dir", required=True)
    p.add_argument("-a", "--annotations_dir", required=True)
    p.add_argument("-o", "--output", required=True)
    p.add_argument("-l", "--labels", required=True)
    p.add_argument("-s", "--num_shards", type=int, default=1)
    p.add_argument("--seed", type=int, default=None, help="the shuffle's seed (default: an unseeded shuffle, as the reference)")
    p.add_argument("--jpeg_device", type=int, default=None, help="re-encode grayscale files on this GPU instead of with PIL")
    args = p.parse_args(argv)
    pool = None
    if args.jpeg_device is not None:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(min(8, os.cpu_count() or 1))
    try:
        counts = create(args.image_dir, args.annotations_dir, args.output, args.labels, args.num_shards, args.seed, args.jpeg_device, pool)
    finally:
        if pool is not None:
            pool.shutdown()
    print("number of images:", counts["examples"])
    print("number of images per shard:", counts["shard_size"])
    print("number of written images:", counts["written"], "in", counts["shards"], "shards")
    print("number of skipped images:", counts["skipped"])
    print("result is here:", args.output)
    return counts


if __name__ == "__main__":
    main()
