"""Drop-in for the reference's inference/detector.py:5-60.

    detector = Detector(model_path)                     # weights .npz (+ config)
    boxes, labels, scores = detector(image_uint8_HW3, score_threshold=0.1)

Same constructor keywords, same return order (boxes, labels, scores), boxes normalised
[ymin, xmin, ymax, xmax].  `model_path` is the reference's frozen graph (`inference/model.pb`), one of the
checkpoints its training leaves behind (a `model.ckpt-N` prefix, the `model_dir`, or the SavedModel directory of
create_pb.py's export/ -- for a user who cannot run create_pb.py without TensorFlow), or this build's own weight
container (a .npz keyed by the reference's TF variable names, see variables.py); the JSON config is the
reference's own file (config_mobilenet.json / config_shufflenet.json).
"""
import json
import os

import numpy as np

from .config import load_config
from .ssd import Engine, _torch, host_frame, mixed_batches, record_batches, score_filter, split_records
from .pb_import import load_pb_weights
from .ckpt_import import load_ckpt_weights, resolve_checkpoint
from .variables import load_weights


def _pil_rgb(blob):
    """The reference notebooks' reader on bytes (inference/just_try_detector.ipynb: PIL, RGB)."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def filtered_records(records, score_threshold):
    """A record block [B, 6T + 1] (a tensor; downloaded here) -> (boxes, labels, scores) of every image at `score_threshold`."""
    boxes, labels, scores, num = split_records(records.cpu().numpy())
    return [score_filter(boxes[i], labels[i], scores[i], num[i], score_threshold) for i in range(len(num))]


class Detector:
    def __init__(self, model_path, gpu_memory_fraction=0.25, visible_device_list='0',
                 config=None, precision=None, use_ema=False):
        """
        Arguments:
            model_path: path to the reference's frozen graph (.pb, read without TensorFlow), to a
                TensorFlow checkpoint of the reference's training (prefix `model.ckpt-N`, its .index /
                .data file, the model_dir with its `checkpoint` state file, or a SavedModel directory:
                ckpt_import.py), to this build's weight file (.npz), or a dict {variable name: ndarray}.
            gpu_memory_fraction: accepted for compatibility and ignored (the library
                allocates exactly the arena the network needs).
            visible_device_list: a string like the reference's; the first entry is the HIP
                device index.
            config: path to the reference's JSON config or a dict; default: `config.json`
                next to `model_path` (the reference reads 'config.json', create_pb.py:18).
            precision: "f32" (every convolution an exact fp32 chain, bit-identical to the CPU
                oracle), "f16x3" (dense convolutions on split-fp16 operands: fp32-chain accuracy,
                2.3x the throughput; should an activation ever leave the fp16 range the call is
                transparently repeated in f32) or None = the library default (SSD_PRECISION
                environment variable, else "f32").
            use_ema: checkpoints only -- take the variables' exponential moving averages (what the
                evaluation inside train.py restores, model.py:148-161) instead of the raw variables (what
                create_pb.py freezes: export_savedmodel restores the checkpoint as it is).
        """
        if isinstance(model_path, dict):
            weights = model_path
            if config is None:
                raise ValueError("config is required when weights are passed as a dict")
        else:
            ckpt = None if str(model_path).endswith((".pb", ".npz")) else resolve_checkpoint(model_path)
            if ckpt is None and not os.path.isfile(model_path):
                raise FileNotFoundError(model_path)       # tf.gfile.GFile would raise too
            if config is None:
                where = model_path if os.path.isdir(model_path) else os.path.dirname(os.path.abspath(model_path))
                config = os.path.join(where, "config.json")
            if ckpt is not None:                           # train.py's model_dir / create_pb.py's export folder
                weights = load_ckpt_weights(ckpt, load_config(config), use_ema=use_ema)
            elif str(model_path).endswith(".pb"):          # the reference's frozen graph (create_pb.py:57-85)
                weights = load_pb_weights(model_path, load_config(config))
            else:
                weights = load_weights(model_path)
        self.params = load_config(config)
        device = int(str(visible_device_list).split(",")[0])
        self.engine = Engine(self.params, weights, device=device, precision=precision)
        self.device = device
        self._config = config
        from .evaluation import l2_sum
        self._l2_sum = l2_sum(weights)       # model.py:132-145 over the loaded (with use_ema: averaged) variables

    def close(self):
        """Frees the engine's device memory (weights, every cached layer plan, staging buffers) now instead of at garbage
        collection; the reference's Detector has no counterpart (its tf.Session lives as long as the object)."""
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _f32_fallback(self, run):
        """run() -- one forward and its results -- and in mode f16x3 the read-and-clear of the status word: when an activation
        exceeded +-65504 and was clamped (ssd_hip.h ssd_status) those results are not trustworthy, so this detector continues in
        the exact mode and run() is repeated.  The caller holds self.engine.lock across this whole call."""
        out = run()
        if self.engine.precision == "f16x3" and self.engine.status() & 1:
            import warnings
            warnings.warn("single-shot-detector_amd: activation outside the fp16 range in precision mode "
                          "f16x3; switching this Detector to f32")
            self.engine.set_precision("f32")
            out = run()
        return out

    def detect_batch(self, images):
        """images: uint8 ndarray [B,H,W,3] (or CUDA tensor), any H, W (the graph's
        resize_keeping_aspect_ratio is fused into the first kernel) -> the graph outputs
        (boxes [B,T,4], labels [B,T], scores [B,T], num_boxes [B]) as numpy arrays
        (model.py:70-73).  Thread-safe, like sess.run on a shared tf.Session (inference/detector.py:34,52)."""
        torch = _torch()
        if isinstance(images, torch.Tensor):
            with self.engine.lock:
                return tuple(t.cpu().numpy() for t in self.engine.forward_cached(images))
        with self.engine.lock:
            return tuple(np.array(v) for v in self._f32_fallback(lambda: self.engine.detect_host(images)))

    def detect_many(self, images, score_threshold=0.1, max_batch=32):
        """`__call__` for a LIST of images of any sizes, batched: the images are grouped by the size the network sees for them
        (resize_keeping_aspect_ratio, pipeline.py:138-194: 480x640, 375x500, 333x500 all become 640x896), every group runs as
        batches of up to `max_batch` frames of DIFFERENT source sizes (ssd_forward_mixed_host: per-frame geometry in the first
        kernel, per-image box_scaler in the last), and the results come back in the order of `images` as (boxes, labels, scores)
        per image -- each bit for bit what `self(image, score_threshold)` returns.  The reference loops one `sess.run` per image
        (inference/evaluate_on_COCO.ipynb:125-150); this is that loop at batch throughput.  Mode f32.
        The batches are ssd.mixed_batches': `max_batch` and its halvings only (one layer plan per network shape and batch size).
        Two batches are in flight: batch k + 1 is staged and uploaded while batch k computes."""
        if self.engine.precision != "f32":
            return [self(im, score_threshold) for im in images]
        imgs = [host_frame(im, "every image") for im in images]
        parts = mixed_batches(self.engine, [im.shape[:2] for im in imgs], max_batch)
        out = [None] * len(imgs)

        def consume(pending):
            slot, part = pending
            slot["done"].synchronize()
            boxes, labels, scores, num = slot["host"]
            for j, i in enumerate(part):
                out[i] = score_filter(boxes[j], labels[j], scores[j], num[j], score_threshold)

        with self.engine.lock:
            pending = None
            for n, part in enumerate(parts):
                slot = self.engine.detect_host_mixed([imgs[i] for i in part], wait=False, index=5 + (n & 1))
                if pending is not None:
                    consume(pending)
                pending = (slot, part)
            if pending is not None:
                consume(pending)
        return out

    def _records_argument(self, name, records, items, convert):
        """The refusals the records routes share, in their order: mode f32; every item taken by `convert` (which refuses its own);
        `records` a tensor on this detector's GPU with len(items) rows of the engine's.  Returns the converted items."""
        torch = _torch()
        if self.engine.precision != "f32":
            raise ValueError("%s runs in precision mode f32 only" % name)
        items = [convert(x) for x in items]
        if not (isinstance(records, torch.Tensor) and records.is_cuda and records.device.index == self.device):
            raise ValueError("records must be a tensor on cuda:%d" % self.device)
        self.engine._check_records(records, len(items))
        return items

    def detect_many_records(self, images, records, max_batch=32):
        """`detect_many` for a caller that keeps the detections on the GPU: the same grouping and the same batches, but the record of
        image i (ssd.split_records) is left UNFILTERED in row i of `records`, a contiguous device int32 tensor [len(images), 6T + 1]
        on this detector's GPU -- bit for bit ssd.pack_records of what detect_many's batches produce.  Nothing is downloaded and
        nothing waits: the forwards and the row copies (ssd.record_batches) are enqueued on the current stream.  Returns `records`.
        Mode f32 only (mode f16x3 needs the per-batch status check of detect_batch): ValueError otherwise."""
        imgs = self._records_argument("detect_many_records", records, images, lambda im: host_frame(im, "every image"))
        with self.engine.lock:
            record_batches(self.engine, [im.shape[:2] for im in imgs], max_batch, records,
                           lambda part, block: self.engine.forward_mixed_host([imgs[i] for i in part], block))
        return records

    # ------------------------------------------------------------------------- from JPEG bytes, decoded on the GPU
    JPEG_GROUP = 256                 # files decoded as one batch of the decoder ..
    JPEG_GROUP_BYTES = 1 << 30       # .. and the frame bytes of one (ssd_forward_mixed addresses 2 GiB from the base)

    def jpeg_decoder(self):
        """This detector's jpeg.JpegDecoder (created on first use)."""
        if getattr(self, "_jpeg", None) is None:
            from .jpeg import JpegDecoder
            self._jpeg = JpegDecoder(self.device)
        return self._jpeg

    def jpeg_encoder(self):
        """This detector's jpeg.JpegEncoder (created on first use)."""
        if getattr(self, "_jpeg_enc", None) is None:
            from .jpeg import JpegEncoder
            self._jpeg_enc = JpegEncoder(self.device)
        return self._jpeg_enc

    def _jpeg_groups(self, blobs):
        """Consecutive index ranges of `blobs`, each within JPEG_GROUP files and JPEG_GROUP_BYTES of frames."""
        dec, groups, start, size = self.jpeg_decoder(), [], 0, 0
        for i, blob in enumerate(blobs):
            rc, info = dec.read_info(blob)
            nbytes = 3 * info.height * info.width + 16 if rc == 0 else 0
            if i > start and (i - start >= self.JPEG_GROUP or size + nbytes > self.JPEG_GROUP_BYTES):
                groups.append((start, i))
                start, size = i, 0
            size += nbytes
        if len(blobs) > start:
            groups.append((start, len(blobs)))
        return groups

    def _jpeg_records(self, batch, records, max_batch, fallback_at):
        """The records of one decoder batch (JpegDecoder.begin's) into `records` [len(batch.blobs), 6T + 1] on this GPU, row for
        row: the accepted files as mixed-size batches straight from the decoded frames, then the refused ones -- fallback_at(index)
        -> ndarray -- as mixed-size batches of host frames, both through ssd.record_batches.  Returns every file's (height, width).
        The caller holds no lock."""
        (flat, hw, offsets), refused = self.jpeg_decoder().finish(batch)
        taken = [i for i in range(len(batch.blobs)) if i not in refused]
        shapes = dict(zip(taken, hw))
        with self.engine.lock:
            record_batches(self.engine, hw, max_batch, records, lambda part, block: self.engine.forward_mixed(
                (flat, [hw[j] for j in part], [offsets[j] for j in part]), block), taken)
        idx = sorted(refused)
        imgs = [host_frame(fallback_at(i), "every image") for i in idx]
        shapes.update((i, tuple(int(v) for v in im.shape[:2])) for i, im in zip(idx, imgs))
        with self.engine.lock:
            record_batches(self.engine, [shapes[i] for i in idx], max_batch, records,
                           lambda part, block: self.engine.forward_mixed_host([imgs[j] for j in part], block), idx)
        return [shapes[i] for i in range(len(batch.blobs))]

    def detect_many_records_jpeg(self, blobs, records, max_batch=32, fallback=None, pool=None):
        """`detect_many_records` for JPEG BYTES: the files are entropy-decoded on the host (on `pool`, a concurrent.futures
        executor, when given) and turned into frames on this GPU (jpeg.JpegDecoder; include/ssd_hip.h "the JPEG decoder"), which
        ssd_forward_mixed reads where they lie -- no decoded frame exists on the host.  Row i of `records` is bit for bit what
        detect_many_records leaves for the PIL-decoded array of blobs[i].  A file the decoder refuses (progressive, CMYK, damaged,
        ..) goes through `fallback(bytes) -> uint8 RGB ndarray` (default: PIL) and the host route.  Group k + 1 of the files is
        entropy-decoded while group k computes.  Returns (records, [(height, width) of every file]).  Mode f32 only."""
        torch = _torch()
        blobs = self._records_argument("detect_many_records_jpeg", records, blobs, lambda b: b if isinstance(b, bytes) else bytes(b))
        fallback = fallback or _pil_rgb
        dec, shapes = self.jpeg_decoder(), []
        with self.engine.lock, torch.cuda.device(self.device):      # (the decoder's two buffers are this detector's: one caller at a time)
            groups = self._jpeg_groups(blobs)
            ahead = dec.begin(blobs[groups[0][0]:groups[0][1]], pool) if groups else None
            for g, (a, b) in enumerate(groups):
                batch = ahead
                ahead = dec.begin(blobs[groups[g + 1][0]:groups[g + 1][1]], pool) if g + 1 < len(groups) else None
                shapes += self._jpeg_records(batch, records[a:b], max_batch, lambda i, a=a: fallback(blobs[a + i]))
        return records, shapes

    def detect_many_jpeg(self, blobs, score_threshold=0.1, max_batch=32, fallback=None, pool=None):
        """`detect_many` for a list of JPEG byte strings, decoded on the GPU (detect_many_records_jpeg): (boxes, labels, scores) per
        file, in order, each bit for bit what `detect_many` returns for the PIL-decoded arrays.  Refused files go through
        `fallback(bytes) -> ndarray` (default: PIL) and the existing host route."""
        fallback = fallback or _pil_rgb
        if self.engine.precision != "f32":
            return self.detect_many([fallback(b) for b in blobs], score_threshold, max_batch)
        records = self.engine.new_records(len(blobs), "cuda:%d" % self.device)
        self.detect_many_records_jpeg(blobs, records, max_batch, fallback, pool)
        return filtered_records(records, score_threshold)

    def detect_tiled(self, image, tile=None, overlap=0.25, full_frame=True, score_threshold=0.1, max_batch=32):
        """`__call__` for a frame much LARGER than the network's input (a 1200 x 1600 camera frame at min_dimension 640), where
        shrinking the frame loses the small objects: the network runs on overlapping tiles of its own size at the frame's own
        resolution, with full_frame also on the shrunk whole frame (the objects larger than a tile), and all records of a frame
        are merged by the detector's own per-class NMS (include/ssd_hip.h, block "tiled detection").
            image: uint8 [H, W, 3] or [F, H, W, 3], a host array or a CUDA tensor.
            tile: a side or (th, tw), multiples of 128 with min(th, tw) == min_dimension (the network sees a tile as it is);
                default: min_dimension square.  H >= th and W >= tw -- a smaller frame is `__call__`'s (ValueError).
            overlap: the fraction of a tile side that neighbouring tiles share.
        Returns (boxes, labels, scores) like `__call__`, boxes normalised to the frame; a list of them for a batch of frames.
        One upload, the gather of the tiles on the device, the tiles' forwards in batches of `max_batch` and its halvings
        (ssd.mixed_batches' rule: one layer plan per batch size), the whole frames' forward, the merge, one download.
        The whole frames run as ONE batch of F whatever `max_batch` says (a layer plan per distinct F): pass a stream of frames
        in groups of one size."""
        from . import tiles as tl
        torch = _torch()
        md = int(self.params["min_dimension"])
        th, tw = (md, md) if tile is None else (tile, tile) if np.isscalar(tile) else tile
        th, tw = int(th), int(tw)
        if th % 128 or tw % 128 or min(th, tw) != md:
            raise ValueError("tile: sides that are multiples of 128 with min(th, tw) == min_dimension (%d)" % md)
        if not isinstance(image, torch.Tensor):
            image = np.asarray(image)
        single = image.ndim == 3
        dtype_ok = image.dtype == (torch.uint8 if isinstance(image, torch.Tensor) else np.uint8)
        if not dtype_ok or image.ndim not in (3, 4) or image.shape[-1] != 3:
            raise ValueError("image must be uint8 of shape [height, width, 3] or [frames, height, width, 3]")
        F, H, W = (1,) + tuple(image.shape[:2]) if single else tuple(image.shape[:3])
        if H < th or W < tw:
            raise ValueError("a %d x %d frame is smaller than the %d x %d tile: use __call__" % (H, W, th, tw))
        ys, xs = tl.tile_grid(H, W, th, tw, overlap)
        n = F * len(ys) * len(xs)
        sizes, b = [], max(1, int(max_batch))
        while b >= 1:
            sizes.append(b)
            b //= 2
        eng = self.engine
        dev = "cuda:%d" % self.device
        with eng.lock:
            frames = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
            frames = frames.to(dev).contiguous().view(F, H, W, 3)
            tiles = tl.tile_gather(frames, th, tw, overlap)
            rec = eng.new_records(n, dev)
            rec_full = eng.new_records(F, dev) if full_frame else None

            def run():
                k = 0
                for b in sizes:
                    while n - k >= b:
                        eng.forward(tiles[k:k + b], records=rec[k:k + b])
                        k += b
                if full_frame:
                    eng.forward(frames, records=rec_full)
                merged = tl.tile_merge(rec, rec_full, (F, H, W), th, tw, overlap, self.params["num_classes"],
                                       self.params["max_boxes_per_class"], self.params["iou_threshold"])
                return merged.cpu().numpy()
            boxes, labels, scores, num = eng.record_views(self._f32_fallback(run))
        out = [score_filter(boxes[f], labels[f], scores[f], num[f], score_threshold) for f in range(F)]
        return out[0] if single else out

    def detect_stream(self, batches):
        """Steady-state serving: an iterable of host uint8 batches [B,H,W,3] -> a generator of the graph outputs per
        batch, in order, with the host-to-device and device-to-host copies of neighbouring batches hidden under the
        compute of the current one (Engine.detect_stream).  Mode f32 (mode f16x3 needs the per-batch status check of
        detect_batch and is served by that method)."""
        if self.engine.precision != "f32":
            for images in batches:
                yield self.detect_batch(images)
            return
        yield from self.engine.detect_stream(batches)

    def regularization_loss(self, weight_decay):
        """model.py:80-81 for the loaded weights: weight_decay * sum of l2_loss over the regularised kernels (float64,
        rounded to float32 once)."""
        return np.float32(float(weight_decay) * self._l2_sum)

    def loss(self, image, boxes, labels, config=None):
        """The EVAL step of train.py for ONE image (model.py:79-104 at batch 1, pipeline.py:22-27): image uint8
        [height, width, 3]; boxes [n,4] ymin,xmin,ymax,xmax normalised to the image, labels [n] in [0, num_classes)
        (create_tfrecords.py's groundtruth).  config: the JSON with the loss keys (config.load_loss_config), default
        the Detector's own.  Returns {'loss' (total_loss), 'localization_loss', 'classification_loss',
        'regularization_loss'} as float32 numbers."""
        from .config import load_loss_config
        from .evaluation import _Run, image_losses
        lc = load_loss_config(self._config if config is None else config)
        image = host_frame(image)
        reg = self.regularization_loss(lc["weight_decay"])
        with self.engine.lock:
            row = _Run(self.engine)([image], [(np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(labels).reshape(-1))], lc)[0][0]
        loc, cls, tot = image_losses(row, reg, lc)
        return {"loss": tot, "localization_loss": loc, "classification_loss": cls, "regularization_loss": reg}

    def __call__(self, image, score_threshold=0.1):
        """
        Arguments:
            image: a numpy uint8 array with shape [height, width, 3] (RGB), or the path of an image file.
            score_threshold: a float number.
        Returns:
            boxes: a float numpy array of shape [N, 4] (ymin, xmin, ymax, xmax!).
            labels: an int numpy array of shape [N].
            scores: a float numpy array of shape [N].
        """
        if isinstance(image, (str, os.PathLike)):
            # BASELINE.json's north star words the API as Detector(image_path): a path is read the way the reference's
            # notebooks read it (inference/just_try_detector.ipynb: PIL, RGB) and then takes the ndarray route
            from PIL import Image
            with Image.open(image) as im:
                image = np.asarray(im.convert("RGB"), dtype=np.uint8)
        image = host_frame(image)
        if self.engine.one_call_detect:
            # one library call: upload, forward, wait and the filter below in C (ssd_detect_host).  The engine's lock (an RLock)
            # is held across the call AND the read-and-clear of the status word: with two threads on one Detector in mode
            # f16x3, thread A's status() must not consume the overflow bit that thread B's forward raised.
            with self.engine.lock:
                return self._f32_fallback(lambda: self.engine.detect_one(image, float(score_threshold)))
        with self.engine.lock:      # the views below live in the engine's pinned result block until the next call
            boxes, labels, scores, n = self._f32_fallback(lambda: self.engine.detect_host(image[None]))
            return score_filter(boxes[0], labels[0], scores[0], n[0], score_threshold)
