"""train.py's input pipeline (pipeline.py:47-64 and the augmentation of :117-135) without TensorFlow.

The host decodes each JPEG and draws the image's random scalars -- the crop window (TF's sample_distorted_bounding_box,
restated below), the colour offsets, the flags, a Philox key -- and does all box arithmetic (a few hundred floats per image).
Every per-pixel step (crop, nearest-neighbour resize, uint8 -> [0, 1], colour, grayscale, per-element scale, flip) runs on the
GPU in one launch per batch (csrc/augment.hip, ssd_augment; semantics in include/ssd_hip.h, block "the TRAIN input
pipeline"), so only uint8 crosses the bus.

TF's random streams cannot be reproduced: what is pinned is the semantics for given draws.  Draws come from a
numpy.random.Generator, in a fixed order per image: crop (probability, then the attempts), colour (probability, brightness,
cb, cr), grayscale, pixel scale (probability, key), four jitter numbers per kept box, flip.
"""
import collections
import ctypes
import time

import numpy as np

from . import tfrecords
from ._lib import check, lib
from .config import load_train_config
from .distributed import read_worker_count

AUG_COLOR, AUG_GRAY, AUG_SCALE, AUG_FLIP = 1, 2, 4, 8          # SSD_AUG_* of include/ssd_hip.h
# ssd_augment_params of include/ssd_hip.h (64 bytes, no padding)
PARAMS_DTYPE = np.dtype([("offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("crop_y", "<i4"), ("crop_x", "<i4"),
                         ("crop_h", "<i4"), ("crop_w", "<i4"), ("flags", "<i4"), ("color_offset", "<f4", (3,)),
                         ("scale_min", "<f4"), ("scale_range", "<f4"), ("philox_key", "<u8")])
assert PARAMS_DTYPE.itemsize == 64

EPSILON = np.float32(1e-8)              # constants.py:12
SHUFFLE_BUFFER_SIZE = 5000              # constants.py:16

# Pipeline.augmentation's hyper-parameters (pipeline.py:120-135)
DEFAULT_SETTINGS = {
    "crop_probability": 0.95, "min_object_covered": 0.5, "aspect_ratio_range": (0.8, 1.2), "area_range": (0.67, 0.97),
    "overlap_thresh": 0.3,
    "color_probability": 0.05, "grayscale_probability": 0.01,
    "scale_minval": 0.85, "scale_maxval": 1.15, "scale_probability": 0.05,
    "jitter_ratio": 0.01,
    "flip_probability": 0.5,
}

_f32 = np.float32


def _unit(rng, size=None):
    """One float32 draw in [0, 1) (or an array of them)."""
    return rng.random(size, dtype=np.float32) if size is not None else _f32(rng.random(dtype=np.float32))


def _uniform(rng, minval, maxval, size=None):
    """tf.random_uniform in float32: u * (maxval - minval) + minval."""
    lo, hi = _f32(minval), _f32(maxval)
    return _unit(rng, size) * (hi - lo) + lo


def _happens(rng, probability):
    """tf.less(tf.random_uniform([]), probability)."""
    return bool(_unit(rng) < _f32(probability))


def _lrint(v):
    """lrintf: float32 rounded to the nearest integer, ties to even."""
    return int(np.rint(_f32(v)))


# ----------------------------------------------------------------------------- the crop window
def _random_crop(rng, H, W, min_area, max_area, ar):
    """GenerateRandomCrop: one attempt at a window of aspect ratio `ar` -> (y, x, h, w) or None."""
    h = _lrint(np.sqrt(min_area / ar))
    max_h = _lrint(np.sqrt(max_area / ar))
    if _lrint(_f32(max_h) * ar) > W:
        max_h = int((W + 0.5 - float(_f32(1e-7))) / float(ar))
    max_h = min(max_h, H)
    if h >= max_h:
        h = max_h
    else:
        h += int(rng.integers(0, max_h - h + 1))
    w = _lrint(_f32(h) * ar)
    area = _f32(w * h)
    if area < min_area:                 # rounding: one retry a pixel taller, then one a pixel shorter
        h += 1
        w = _lrint(_f32(h) * ar)
        area = _f32(w * h)
    if area > max_area:
        h -= 1
        w = _lrint(_f32(h) * ar)
        area = _f32(w * h)
    if area < min_area or area > max_area or w > W or h > H or w <= 0 or h <= 0:
        return None
    y = int(rng.integers(0, H - h)) if h < H else 0
    x = int(rng.integers(0, W - w)) if w < W else 0
    return y, x, h, w


def _covers(win, rects, min_object_covered):
    """SatisfiesOverlapConstraints: some box of at least one pixel has intersection / area >= min_object_covered."""
    y, x, h, w = win
    if h * w < 1:
        return False
    for ry0, rx0, ry1, rx1 in rects:
        area = (ry1 - ry0) * (rx1 - rx0)
        if ry1 - ry0 <= 0 or rx1 - rx0 <= 0 or area < 1:
            continue
        ih = min(y + h, ry1) - max(y, ry0)
        iw = min(x + w, rx1) - max(x, rx0)
        inter = ih * iw if ih > 0 and iw > 0 else 0
        if _f32(inter) / _f32(area) >= _f32(min_object_covered):
            return True
    return False


def sample_distorted_bounding_box(rng, height, width, boxes, min_object_covered, aspect_ratio_range, area_range,
                                  max_attempts=100):
    """tf.image.sample_distorted_bounding_box of TF 1.12 with use_image_if_no_bounding_boxes=True -> the integer window
    (y, x, h, w).  A restatement of TF's algorithm as recalled, not read from its source: per attempt an aspect ratio
    uniform in the range; height = lrint(sqrt(min_area / ar)), max_height = lrint(sqrt(max_area / ar)), lowered to
    (int)((W + 0.5 - 1e-7) / ar) when lrint(max_height * ar) > W and clamped to H; height uniform in [height, max_height],
    width = lrint(height * ar); one retry at height + 1 when the area falls below min_area, one at height - 1 when it
    exceeds max_area; the attempt fails when the area is still out of range or the window does not fit or is empty;
    otherwise y uniform in [0, H - h), x in [0, W - w).  It is accepted when some box of positive pixel area (boxes
    become int32(coordinate * size) pixel rectangles; no boxes: the whole image) is covered >= min_object_covered.  No
    accepted attempt: the whole image.  Areas are float32 as in TF; boxes: normalised [n, 4] ymin, xmin, ymax, xmax."""
    H, W = int(height), int(width)
    rects = [(int(b[0] * _f32(H)), int(b[1] * _f32(W)), int(b[2] * _f32(H)), int(b[3] * _f32(W)))
             for b in np.asarray(boxes, np.float32).reshape(-1, 4)]
    if not rects:
        rects = [(0, 0, H, W)]
    min_area = _f32(area_range[0]) * _f32(W) * _f32(H)
    max_area = _f32(area_range[1]) * _f32(W) * _f32(H)
    for _ in range(max_attempts):
        ar = _uniform(rng, aspect_ratio_range[0], aspect_ratio_range[1])
        win = _random_crop(rng, H, W, min_area, max_area, ar)
        if win is not None and _covers(win, rects, min_object_covered):
            return win
    return 0, 0, H, W


# ----------------------------------------------------------------------------- box steps (random_image_crop.py, float32)
def area(boxes):
    """box_utils.py:53-62."""
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def intersection(boxes1, boxes2):
    """box_utils.py:30-50: pairwise intersection areas [N, M]."""
    h = np.maximum(_f32(0), np.minimum(boxes1[:, None, 2], boxes2[None, :, 2]) - np.maximum(boxes1[:, None, 0], boxes2[None, :, 0]))
    w = np.maximum(_f32(0), np.minimum(boxes1[:, None, 3], boxes2[None, :, 3]) - np.maximum(boxes1[:, None, 1], boxes2[None, :, 1]))
    return h * w


def ioa(boxes1, boxes2):
    """random_image_crop.py:195-211: intersection / (area(boxes2) + EPSILON), clipped to [0, 1]: [N, M]."""
    return np.clip(intersection(boxes1, boxes2) / (area(boxes2)[None, :] + EPSILON), _f32(0), _f32(1))


def prune_completely_outside_window(boxes, window):
    """random_image_crop.py:113-143 -> (boxes, kept indices)."""
    bad = ((boxes[:, 0] >= window[2]) | (boxes[:, 1] >= window[3]) | (boxes[:, 2] <= window[0]) | (boxes[:, 3] <= window[1]))
    keep = np.nonzero(~bad)[0]
    return boxes[keep], keep


def prune_non_overlapping_boxes(boxes, window, min_overlap):
    """random_image_crop.py:146-170 for one window: keep the boxes whose IOA with it is >= min_overlap."""
    keep = np.nonzero(ioa(window[None, :], boxes).reshape(-1) >= _f32(min_overlap))[0]
    return boxes[keep], keep


def change_coordinate_frame(boxes, window):
    """random_image_crop.py:173-192: coordinates relative to the window, clipped to [0, 1]."""
    wh, ww = window[2] - window[0], window[3] - window[1]
    out = np.stack([(boxes[:, 0] - window[0]) / wh, (boxes[:, 1] - window[1]) / ww,
                    (boxes[:, 2] - window[0]) / wh, (boxes[:, 3] - window[1]) / ww], axis=1)
    return np.clip(out, _f32(0), _f32(1)).astype(np.float32).reshape(-1, 4)


def jitter_boxes(boxes, rand):
    """random_jitter_boxes (other_augmentations.py:112-150) for given draws rand [n, 4] in [-ratio, ratio)."""
    h, w = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    return np.clip(boxes + np.stack([h, w, h, w], axis=1) * rand, _f32(0), _f32(1)).astype(np.float32).reshape(-1, 4)


def flip_boxes(boxes):
    """random_flip_left_right's boxes (other_augmentations.py:57-63)."""
    one = _f32(1)
    return np.stack([boxes[:, 0], one - boxes[:, 3], boxes[:, 2], one - boxes[:, 1]], axis=1).astype(np.float32).reshape(-1, 4)


def color_offsets(br_delta, cb_factor, cr_factor):
    """random_color_manipulations' channel offsets (other_augmentations.py:16-28) in float32, in the reference's order."""
    br, cb, cr = _f32(br_delta), _f32(cb_factor), _f32(cr_factor)
    red = _f32(1.402) * cr + br
    green = _f32(-0.344136) * cb - _f32(0.714136) * cr + br
    blue = _f32(1.772) * cb + br
    return np.array([red, green, blue], np.float32)


def sample_augmentation(rng, height, width, boxes, labels, settings=None):
    """Pipeline.augmentation (pipeline.py:117-135) for one image of `height` x `width`: the draws, and all box work.
    boxes: normalised [n, 4] (ymin, xmin, ymax, xmax), labels [n].  Returns (params, boxes, labels): one ssd_augment_params
    row (PARAMS_DTYPE; offset 0, frame size = height x width) and the image's boxes (float32 [k, 4], normalised to the
    output image) and labels (int32 [k]) after the augmentation.  settings: DEFAULT_SETTINGS, or a dict overriding some."""
    s = dict(DEFAULT_SETTINGS, **(settings or {}))
    H, W = int(height), int(width)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    labels = np.asarray(labels, np.int32).reshape(-1)
    if len(labels) != len(boxes):
        raise ValueError("boxes and labels differ in length")
    p = np.zeros((), PARAMS_DTYPE)
    p["height"], p["width"] = H, W
    y, x, h, w = 0, 0, H, W
    if _happens(rng, s["crop_probability"]):                                            # random_image_crop
        y, x, h, w = sample_distorted_bounding_box(rng, H, W, boxes, s["min_object_covered"], s["aspect_ratio_range"],
                                                   s["area_range"])
        window = np.array([_f32(y) / _f32(H), _f32(x) / _f32(W), _f32(y + h) / _f32(H), _f32(x + w) / _f32(W)], np.float32)
        boxes, inside = prune_completely_outside_window(boxes, window)
        boxes, keep = prune_non_overlapping_boxes(boxes, window, s["overlap_thresh"])
        boxes = change_coordinate_frame(boxes, window)
        labels = labels[inside[keep]]
    p["crop_y"], p["crop_x"], p["crop_h"], p["crop_w"] = y, x, h, w
    flags = 0
    if _happens(rng, s["color_probability"]):                                           # random_color_manipulations
        br = _uniform(rng, -32.0 / 255.0, 32.0 / 255.0)
        cb = _uniform(rng, -0.1, 0.1)
        cr = _uniform(rng, -0.1, 0.1)
        p["color_offset"] = color_offsets(br, cb, cr)
        flags |= AUG_COLOR
    if _happens(rng, s["grayscale_probability"]):
        flags |= AUG_GRAY
    if _happens(rng, s["scale_probability"]):                                           # random_pixel_value_scale
        p["philox_key"] = rng.integers(0, 2 ** 64, dtype=np.uint64)
        flags |= AUG_SCALE
    p["scale_min"] = _f32(s["scale_minval"])
    p["scale_range"] = _f32(s["scale_maxval"]) - _f32(s["scale_minval"])
    boxes = jitter_boxes(boxes, _uniform(rng, -s["jitter_ratio"], s["jitter_ratio"], (len(boxes), 4)))   # random_jitter_boxes
    if _happens(rng, s["flip_probability"]):                                            # random_flip_left_right
        boxes = flip_boxes(boxes)
        flags |= AUG_FLIP
    p["flags"] = flags
    return p[()], boxes, labels.astype(np.int32)


# ----------------------------------------------------------------------------- the batch on the GPU
def _torch():
    from .ssd import _torch as t
    return t()


def _check_windows(params, shapes):
    for b, (p, (h, w)) in enumerate(zip(params, shapes)):
        if (p["crop_h"] < 1 or p["crop_w"] < 1 or p["crop_y"] < 0 or p["crop_x"] < 0 or p["crop_y"] + p["crop_h"] > h
                or p["crop_x"] + p["crop_w"] > w):
            raise ValueError("image %d: empty or out-of-frame crop window" % b)


def augment_batch(frames, params, out_hw, channels_first=False):
    """The per-pixel half of Pipeline.augmentation for a batch (ssd_augment): frames, a list of uint8 [H, W, 3] arrays
    (numpy) or CUDA tensors (one device); params: their ssd_augment_params rows (sample_augmentation; offset, height and
    width are taken from the frames).  Returns the CUDA float32 batch [B, out_h, out_w, 3] ([B, 3, out_h, out_w] with
    channels_first), asynchronous on the current stream.  Host frames: only each crop window is staged, with the rows, into
    one pinned buffer and crosses the bus in one copy.  CUDA frames are read where they lie."""
    torch = _torch()
    B = len(frames)
    params = np.array(params, PARAMS_DTYPE).reshape(-1)
    if B < 1 or len(params) != B:
        raise ValueError("augment_batch needs one params row per frame (and at least one frame)")
    out_h, out_w = (int(v) for v in out_hw)
    on_dev = [isinstance(f, torch.Tensor) and f.is_cuda for f in frames]
    for f in frames:
        if tuple(f.shape[2:]) != (3,) or len(f.shape) != 3 or f.dtype not in (np.uint8, torch.uint8):
            raise TypeError("frames must be uint8 [H, W, 3]")
    _check_windows(params, [f.shape[:2] for f in frames])
    if all(on_dev):
        dev = frames[0].device
        if any(f.device != dev or not f.is_contiguous() for f in frames):
            raise ValueError("CUDA frames must be contiguous and on one device")
        ptrs = [f.data_ptr() for f in frames]
        base = min(ptrs)
        params["offset"] = [q - base for q in ptrs]
        params["height"] = [f.shape[0] for f in frames]
        params["width"] = [f.shape[1] for f in frames]
        staged = torch.from_numpy(params.view(np.uint8)).pin_memory()
        params_dev = staged.to(dev, non_blocking=True)
        images_dev = ctypes.c_void_p(base)
    elif not any(on_dev):
        dev = torch.device("cuda", torch.cuda.current_device())
        head = 64 * B
        sizes = [int(p["crop_h"]) * int(p["crop_w"]) * 3 for p in params]
        offs = np.concatenate([[0], np.cumsum([(n + 15) & ~15 for n in sizes])]).astype(np.int64)
        staged = torch.empty((head + int(offs[-1]),), dtype=torch.uint8, pin_memory=True)
        arr = staged.numpy()
        for b, (f, p) in enumerate(zip(frames, params)):
            y, x, h, w = int(p["crop_y"]), int(p["crop_x"]), int(p["crop_h"]), int(p["crop_w"])
            o = head + int(offs[b])
            np.copyto(arr[o:o + h * w * 3].reshape(h, w, 3), np.asarray(f)[y:y + h, x:x + w])
        params["offset"] = offs[:-1]
        params["height"], params["width"] = params["crop_h"], params["crop_w"]
        params["crop_y"], params["crop_x"] = 0, 0
        arr[:head] = params.view(np.uint8)
        params_dev = staged.to(dev, non_blocking=True)                 # rows and crops: one upload
        images_dev = ctypes.c_void_p(params_dev.data_ptr() + head)
    else:
        raise TypeError("frames must be all numpy arrays or all CUDA tensors")
    shape = (B, 3, out_h, out_w) if channels_first else (B, out_h, out_w, 3)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    check(lib().ssd_augment(images_dev, params.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(params_dev.data_ptr()), B,
                            out_h, out_w, 1 if channels_first else 0, ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


# ----------------------------------------------------------------------------- the record stream
def shuffle_buffer(items, size, rng):
    """tf.data's shuffle(buffer_size=size): fill the buffer, emit a uniformly drawn slot and refill that slot; at the end
    of the input, drain the buffer in uniform order."""
    buf = []
    for it in items:
        if len(buf) < size:
            buf.append(it)
            continue
        i = int(rng.integers(len(buf)))
        out, buf[i] = buf[i], it
        yield out
    while buf:
        i = int(rng.integers(len(buf)))
        buf[i], buf[-1] = buf[-1], buf[i]
        yield buf.pop()


class TrainPipeline:
    """Pipeline(filenames, is_training=True, params) of pipeline.py:10-64: an iterator over (images, groundtruth) --
    images the CUDA float32 batch [batch_size, image_height, image_width, 3] ([.., 3, h, w] with channels_first),
    groundtruth = {'boxes' [B, G, 4], 'labels' [B, G], 'num_boxes' [B]} as CUDA tensors: what ssd_loss,
    get_training_targets and differentiable_loss take.

    dataset_path: a directory of .tfrecords shards (or one shard); config: the reference's JSON (path or dict;
    load_train_config).  Per epoch the shards come in a fresh random order, their records pass TF's 5 000-slot shuffle
    buffer, and the stream repeats forever (`epochs`: stop after that many); batches drop the remainder.  G is the
    batch's largest box count, at least 1 (zero rows pad).  JPEGs are decoded on `read_workers` threads (default
    min(16, CPUs)) ahead of the consumer; `decode` (JPEG bytes -> uint8 [H, W, 3]) replaces PIL.  Every random draw is
    made by the consumer in stream order from generators seeded by `seed` (one for the record order, one for the
    augmentation): the stream is the same for a seed whatever read_workers is.  While the caller runs step k, batch k + 1
    is uploaded and augmented on a side stream; the caller's current stream waits for it through an event.
    `wait_seconds` accumulates the time the consumer blocked on a decode.
    `shard` = (rank, world): this pipeline keeps shards[rank::world] of the sorted shard list (data-parallel training: every
    rank reads its own files); a rank that would get none is a ValueError.  None: every shard."""

    def __init__(self, dataset_path, config, seed, decode=None, read_workers=None, device=0, channels_first=False,
                 epochs=None, settings=None, shard=None):
        cfg = load_train_config(config)
        self.batch_size = cfg["batch_size"]
        self.out_hw = (cfg["image_height"], cfg["image_width"])
        self.shards = tfrecords.shard_paths(dataset_path)
        if not self.shards:
            raise ValueError("no .tfrecords shards in %r" % (dataset_path,))
        if shard is not None:
            rank, world = (int(v) for v in shard)
            if world < 1 or not 0 <= rank < world:
                raise ValueError("shard must be (rank, world) with 0 <= rank < world, got %r" % (shard,))
            mine = sorted(self.shards)[rank::world]
            if not mine:
                raise ValueError("rank %d of %d gets no shard: %r holds %d" % (rank, world, dataset_path, len(self.shards)))
            self.shards = mine
        order_seq, aug_seq = np.random.SeedSequence(seed).spawn(2)
        self.order_rng = np.random.default_rng(order_seq)
        self.aug_rng = np.random.default_rng(aug_seq)
        self.decode = decode or tfrecords.decode_image
        self.read_workers = read_worker_count(read_workers)
        self.device = int(device)
        self.channels_first = bool(channels_first)
        self.epochs = epochs
        self.settings = settings
        self.wait_seconds = 0.0
        self._gen = None

    def records(self):
        """The raw record stream: shards in a fresh permutation per epoch, then the shuffle buffer (pipeline.py:47-57)."""
        epoch = 0
        while self.epochs is None or epoch < self.epochs:
            order = self.order_rng.permutation(len(self.shards))
            count = 0
            for r in shuffle_buffer((r for i in order for r in tfrecords.read_records(self.shards[i])), SHUFFLE_BUFFER_SIZE,
                                    self.order_rng):
                count += 1
                yield r
            if count == 0:
                raise ValueError("the training dataset is empty")
            epoch += 1

    def _load(self, record):
        jpeg, boxes, labels = tfrecords.read_example(record)
        frame = np.asarray(self.decode(jpeg))
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("decode must return uint8 [H, W, 3]")
        return np.ascontiguousarray(frame), boxes, labels

    def host_batches(self):
        """The host half, without a GPU: lists of batch_size (frame, params row, boxes, labels) in stream order."""
        ahead = 2 * self.batch_size + self.read_workers
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=self.read_workers) as pool:
            recs = self.records()
            pending = collections.deque()

            def fill():
                while len(pending) < ahead:
                    r = next(recs, None)
                    if r is None:
                        return
                    pending.append(pool.submit(self._load, r))
            fill()
            batch = []
            while pending:
                fut = pending.popleft()
                fill()
                t0 = time.perf_counter()
                frame, boxes, labels = fut.result()
                self.wait_seconds += time.perf_counter() - t0
                p, bx, lb = sample_augmentation(self.aug_rng, frame.shape[0], frame.shape[1], boxes, labels, self.settings)
                batch.append((frame, p, bx, lb))
                if len(batch) == self.batch_size:
                    yield batch
                    batch = []

    @staticmethod
    def groundtruth(batch):
        """padded_batch's boxes / labels / num_boxes (numpy) of one host batch: zero rows pad to the largest count, >= 1."""
        G = max(1, max(len(lb) for _f, _p, _b, lb in batch))
        boxes = np.zeros((len(batch), G, 4), np.float32)
        labels = np.zeros((len(batch), G), np.int32)
        num = np.zeros((len(batch),), np.int32)
        for i, (_f, _p, bx, lb) in enumerate(batch):
            boxes[i, :len(lb)], labels[i, :len(lb)], num[i] = bx, lb, len(lb)
        return {"boxes": boxes, "labels": labels, "num_boxes": num}

    def _batches(self):
        torch = _torch()
        dev = torch.device("cuda", self.device)
        side = torch.cuda.Stream(device=dev)
        host = self.host_batches()

        def enqueue():
            batch = next(host, None)
            if batch is None:
                return None
            with torch.cuda.device(dev), torch.cuda.stream(side):
                images = augment_batch([f for f, _p, _b, _l in batch], [p for _f, p, _b, _l in batch], self.out_hw,
                                       self.channels_first)
                gt = {k: torch.from_numpy(v).pin_memory().to(dev, non_blocking=True)
                      for k, v in self.groundtruth(batch).items()}
                ready = torch.cuda.Event()
                ready.record(side)
            return images, gt, ready

        nxt = enqueue()
        while nxt is not None:
            images, gt, ready = nxt
            nxt = enqueue()                                     # batch k + 1 goes to the GPU before the caller's step k
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ready)
            images.record_stream(cur)
            for t in gt.values():
                t.record_stream(cur)
            yield images, gt

    def __iter__(self):
        return self

    def __next__(self):
        if self._gen is None:
            self._gen = self._batches()
        return next(self._gen)
