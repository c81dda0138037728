"""COCO val2017 evaluation harness around `Detector` -- the product-side mirror of the
reference's inference/evaluate_on_COCO.ipynb (cells 6-17) -- and the VOC-style AP@IoU
self-check of the reference's metrics.py:156-282 (`Evaluator`, `evaluate_detector`).
No COCO images or annotations exist offline, so the tests run the harness on synthetic scenes;
`evaluate` needs the dataset on disk and nothing else: the COCO statistics of cell 17 come from
coco_metric.py, this build's restatement of pycocotools' COCOeval for boxes.

Label ids: the detector's integer label i is line i of the reference's data/coco_labels.txt,
which is the standard 80-name COCO order (COCO_NAMES below); the official category ids come
from the annotation file (name -> id), exactly as cell 7 builds `integer_to_coco_id`.
"""
import json
import os

import numpy as np

COCO_NAMES = [
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
    "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant",
    "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard",
    "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle",
    "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange", "broccoli",
    "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed", "dining table", "toilet",
    "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink",
    "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush"]


def integer_to_coco_id(categories):
    """categories: coco.loadCats(coco.getCatIds()) -> {detector label: official category id}
    (evaluate_on_COCO.ipynb cell 7)."""
    labels = {n: i for i, n in enumerate(COCO_NAMES)}
    return {labels[c["name"]]: c["id"] for c in categories}


def result_rows(hw, image_id, label_to_coco_id, detections):
    """One image's (boxes, labels, scores) -> COCO result dicts, exactly as cell 10: boxes scaled to pixels of the ORIGINAL image
    of (height, width) `hw`, x, y = int(xmin), int(ymin); w, h = int(xmax - xmin), int(ymax - ymin)."""
    height, width = hw
    boxes, labels, scores = detections
    scaler = np.array([height, width, height, width], dtype="float32")
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4) * scaler
    # cell 10 per detection: x, y = int(xmin), int(ymin); w, h = int(xmax - xmin), int(ymax - ymin) on float32 values -- the same
    # float32 differences and truncations toward zero, for all rows at once
    x, y = boxes[:, 1].astype(np.int64).tolist(), boxes[:, 0].astype(np.int64).tolist()
    w, h = (boxes[:, 3] - boxes[:, 1]).astype(np.int64).tolist(), (boxes[:, 2] - boxes[:, 0]).astype(np.int64).tolist()
    cats = [int(label_to_coco_id[int(l)]) for l in np.asarray(labels).reshape(-1).tolist()]
    sc = np.asarray(scores, np.float32).reshape(-1).astype(np.float64).tolist()         # float(np.float32) per element
    image_id = int(image_id)
    return [{"image_id": image_id, "category_id": c, "bbox": [xi, yi, wi, hi], "score": s} for c, xi, yi, wi, hi, s in zip(cats, x, y, w, h, sc)]


def detection_records(detector, image, image_id, label_to_coco_id, score_threshold=0.15, detections=None):
    """One image -> COCO result dicts (result_rows).  `detections` = (boxes, labels, scores) already computed for this image (a
    batched run), else the detector is called."""
    height, width, _ = image.shape
    if detections is None:
        detections = detector(image, score_threshold=score_threshold)
    return result_rows((height, width), image_id, label_to_coco_id, detections)


def _rows_of(image_ids, shapes, detections, label_to_coco_id):
    return [row for image_id, hw, d in zip(image_ids, shapes, detections) for row in result_rows(hw, image_id, label_to_coco_id, d)]


def detection_records_many(detector, images, image_ids, label_to_coco_id, score_threshold=0.15, max_batch=32):
    """The same for a list of images of any sizes, with the detector's batched form when it has one (Detector.detect_many: images
    grouped by the size the network sees, frames of different source sizes in one batch; each result bit for bit the single call's)."""
    dets, shapes = _HostChunk(None, images).detections(detector, score_threshold, max_batch)
    return _rows_of(image_ids, shapes, dets, label_to_coco_id)


class _HostChunk:
    """A chunk of evaluate(): the metas of consecutive images and the images themselves, decoded on the host."""

    def __init__(self, metas, images):
        self.metas, self.images = metas, images

    def records_into(self, detector, block, max_batch):
        """Every image's unfiltered record into its row of `block`, a record block on the detector's GPU (nothing waits) -> the
        images' (height, width)."""
        detector.detect_many_records(self.images, block, max_batch=max_batch)
        return [im.shape[:2] for im in self.images]

    def detections(self, detector, score_threshold, max_batch):
        """-> ((boxes, labels, scores) per image, the images' (height, width)): Detector.detect_many, or one call per image of
        a detector that has no batched form."""
        many = getattr(detector, "detect_many", None)
        dets = (many(self.images, score_threshold=score_threshold, max_batch=max_batch) if many
                else [detector(im, score_threshold=score_threshold) for im in self.images])
        return dets, [im.shape[:2] for im in self.images]


class _JpegChunk:
    """The same chunk as a batch of the detector's JPEG decoder (JpegDecoder.begin's): the frames come into being on the GPU and
    are detected where they lie; a file the decoder refuses is read from `images_dir` with `read_image` and takes the host route."""

    def __init__(self, metas, batch, images_dir, read_image):
        self.metas, self.batch, self.images_dir, self.read_image = metas, batch, images_dir, read_image

    def _fallback_at(self, i):
        return self.read_image(os.path.join(self.images_dir, self.metas[i]["file_name"]))

    def records_into(self, detector, block, max_batch):
        return detector._jpeg_records(self.batch, block, max_batch, self._fallback_at)

    def detections(self, detector, score_threshold, max_batch):
        from .detector import filtered_records
        block = detector.engine.new_records(len(self.metas), "cuda:%d" % detector.device)
        shapes = self.records_into(detector, block, max_batch)
        return filtered_records(block, score_threshold), shapes


def evaluate(detector, annotations_json, images_dir, read_image=None, predictions_json="coco_predictions.json", out=None,
             score_threshold=0.15, max_batch=32, read_workers=None, group=None, chunk=256, metric_device=None, rows_device=None,
             jpeg_device=None):
    """Cells 4-17 end to end: every image of the annotation file through the detector (score_threshold 0.15, cell 10), the
    results written as `predictions_json` (cell 11), then the twelve COCO box statistics (cell 17: COCOeval over all image and
    category ids) -- computed by coco_metric.py, this build's restatement of pycocotools' COCOeval (not installed here, not
    vendored by the reference).  `annotations_json`: path of instances_val2017.json or its dict; `read_image(path) -> uint8 RGB
    ndarray`, default PIL (the notebook reads with cv2 and converts BGR -> RGB: the same array when both decoders are built on the
    same libjpeg, which is the usual case but nothing here can check; pass the notebook's reader to be sure); `out`: a stream for
    the summary table; `read_workers`: threads that read and decode images (default min(16, CPUs): a JPEG decodes in ~5 ms on
    one core, the detector takes ~1.4 ms per image in batches -- the next chunk of files is decoded while this one is detected).
    Returns the statistics in coco_metric.STAT_NAMES order (AP, AP50, AP75, APs, APm, APl, AR1, ...).

    `group`: a torch.distributed process group to shard the images over (None: this process does everything).  The images,
    sorted by id, go to the ranks in round-robin chunks of `chunk` (distributed.ChunkAssignment); each rank reads, decodes and
    detects only its own, builds their result rows and runs the per-(image, category, area) matching for them
    (CocoBoxEval.evaluate(img_ids)); one all-gather of compact arrays (the matching cells, the rows' JSON bytes) follows.  Rank
    0 writes `predictions_json` (byte for byte the one-process file) and the table; every rank returns the same statistics.

    `metric_device`: None runs that matching and the accumulation behind it as coco_metric's host loops; a CUDA device index or
    torch.device runs each as one launch on that GPU (CocoBoxEval.evaluate(device=, unpack=False), accumulate(device=)): the same
    cells, precision and recall arrays bit for bit, so the statistics are unchanged.  One process never builds eval_imgs then; with
    `group` the cells still travel as `cells()`, and every rank accumulates the merged cells on its own `metric_device`.

    `rows_device`: None builds the result dicts as above; a CUDA device index or torch.device -- the detector's GPU; `metric_device`
    must be None or the same device (ValueError) and is taken to be it -- never builds them: the detector leaves every image's
    record on that GPU (Detector.detect_many_records), the metric's rows are built there from the records
    (CocoBoxEval.from_records; include/ssd_hip.h "the COCO rows") and matched and accumulated there, and the predictions file is
    formatted from the downloaded records per chunk (coco_rows.write_predictions).  The same statistics and the same file, byte for
    byte.  With `group` every rank builds the rows of its own images; the cells travel as before.

    `jpeg_device`: None reads and decodes every file with `read_image` as above; a CUDA device index or torch.device -- the
    detector's GPU (ValueError otherwise) -- reads the files' BYTES instead, runs the entropy stage of the JPEG decoder on the
    reader threads and turns the coefficients into frames on the GPU, where the detector reads them (Detector.detect_many_records_jpeg's
    core; include/ssd_hip.h "the JPEG decoder"): chunk k + 1 is read and entropy-decoded while chunk k is detected.  A file the
    decoder refuses (progressive, CMYK, not a JPEG, ..) is read with `read_image` and takes the host route.  The frames are PIL's
    bit for bit, so with the default reader the statistics and the predictions file are the same, byte for byte; combinable with
    `rows_device` and `metric_device`.  A chunk's frames must stay below 2 GiB (256 files of 1600 x 1600).

    Either way the images arrive as chunk objects (_HostChunk, _JpegChunk: `metas`, `records_into`, `detections`) from
    _read_chunks, and the loops below do not know which."""
    from . import coco_metric
    from .distributed import ChunkAssignment, read_worker_count
    if read_image is None:
        from PIL import Image

        def read_image(path):
            return np.asarray(Image.open(path).convert("RGB"))
    gt = json.load(open(annotations_json)) if isinstance(annotations_json, str) else annotations_json
    mapping = integer_to_coco_id(gt["categories"])
    metas = sorted(gt["images"], key=lambda m: m["id"])
    if group is None:
        world, rank = 1, 0
    else:
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    mine = [m for _i, m in ChunkAssignment(world, rank, chunk).select(metas)]
    ids = [m["id"] for m in mine]
    if jpeg_device is not None:
        from .detector import Detector
        from .metric_calls import device_of
        if not isinstance(detector, Detector) or device_of(jpeg_device).index != detector.device:
            raise ValueError("jpeg_device must be the GPU of a Detector: the frames are detected where they are decoded")
    if rows_device is not None:
        from .metric_calls import device_of
        dev = device_of(rows_device)
        if metric_device is not None and device_of(metric_device) != dev:
            raise ValueError("metric_device must be None or rows_device (%s): the rows are matched where they are built" % dev)
        metric_device = dev
    workers = read_worker_count(read_workers)
    if jpeg_device is None:
        # chunk k + 1 is being read and decoded while chunk k is consumed (PIL and cv2 release the interpreter lock while they decode)
        chunks = _read_chunks(mine, images_dir, workers, chunk, read_image, 0,
                              lambda part, files, pool: _HostChunk(part, [f.result() for f in files]))
    else:
        # the threads read the files' bytes and run the decoder's entropy stage (plain C behind ctypes: the interpreter lock is
        # released): chunk k + 1 is being entropy-decoded while chunk k is consumed, and the files of chunk k + 2 are being read
        dec = detector.jpeg_decoder()
        chunks = _read_chunks(mine, images_dir, workers, chunk, _read_file, 1, lambda part, files, pool: _JpegChunk(
            part, dec.begin([f.result() for f in files], pool), images_dir, read_image))
    frags = []
    if rows_device is not None:
        import torch
        with torch.cuda.device(dev):
            ev = _evaluate_records(detector, gt, chunks, ids, mapping, score_threshold, max_batch, dev, frags if predictions_json else None)
    else:
        results = []
        for c in chunks:
            # images read, then detected as batches grouped by network shape (the notebook's loop, one image per sess.run, at batch throughput)
            dets, shapes = c.detections(detector, score_threshold, max_batch)
            rows = _rows_of([m["id"] for m in c.metas], shapes, dets, mapping)
            results += rows
            if predictions_json:
                frags.append(json.dumps(rows)[1:-1].encode())      # json.dump of the whole list joins these with ", "
        ev = coco_metric.CocoBoxEval(gt, results)
        ev.evaluate(img_ids=ids, device=metric_device, unpack=False)
    return _finish(ev, frags, metas, chunk, group, world, rank, predictions_json, out, metric_device)


def _evaluate_records(detector, gt, chunks, ids, mapping, score_threshold, max_batch, dev, frags):
    """evaluate()'s detection and matching of the images `ids`, chunk by chunk, without a result dict: -> the evaluated CocoBoxEval
    (outputs on `dev`); the predictions file's fragment of every chunk is appended to `frags` unless that is None."""
    from . import coco_metric, coco_rows
    records = detector.engine.new_records(len(ids), dev)
    shapes, k = [], 0
    for c in chunks:
        block = records[k:k + len(c.metas)]
        shapes += c.records_into(detector, block, max_batch)
        if frags is not None:
            frags.append(coco_rows.write_predictions(block.cpu().numpy(), ids[k:k + len(c.metas)], shapes[k:], mapping, score_threshold))
        k += len(c.metas)
    ev = coco_metric.CocoBoxEval.from_records(gt, records, ids, mapping, score_threshold, device=dev, image_hw=shapes)
    ev.evaluate(img_ids=ids, device=dev, unpack=False)
    return ev


def _finish(ev, frags, metas, chunk, group, world, rank, predictions_json, out, metric_device):
    """evaluate() behind the matching: the ranks' exchange, the predictions file, the accumulation and the table."""
    from .distributed import ChunkAssignment
    if group is not None:
        import torch.distributed as dist
        # one all-gather of every rank's matching cells and its chunks' JSON; the chunks go back in input order (chunk c of the
        # sorted images is rank c % world's: a round-robin split in chunks of one)
        payload = {"cells": ev.cells(), "json": np.frombuffer(b"".join(frags), np.uint8),
                   "lens": np.array([len(f) for f in frags], np.int64)}
        got = [None] * world
        dist.all_gather_object(got, payload, group=group)
        per_rank = []
        for r, p in enumerate(got):
            if r != rank:
                ev.merge(p["cells"])
            blob, ends = p["json"].tobytes(), np.cumsum(p["lens"]).tolist()
            per_rank += [blob[a:b] for a, b in zip([0] + ends[:-1], ends)]
        if predictions_json:
            chunks = ChunkAssignment(world, 0, 1)
            frags = chunks.to_input_order(per_rank, [chunks.count(-(-len(metas) // chunk), r) for r in range(world)])
    if predictions_json and rank == 0:
        with open(predictions_json, "wb") as f:
            f.write(b"[" + b", ".join(x for x in frags if x) + b"]")
    return ev.accumulate(device=metric_device).summarize(out if rank == 0 else None)


def _read_file(path):
    with open(path, "rb") as f:
        return f.read()


def _read_chunks(metas, images_dir, workers, chunk, read, ahead, build):
    """The chunk objects of consecutive chunks of `metas`, on one thread pool: read(path) runs on the pool for every file of a
    chunk, build(the chunk's metas, those futures, the pool) makes its object.  Chunk k + ahead is built and the reads of chunk
    k + ahead + 1 are submitted just before chunk k is handed out, so they proceed while the caller works on chunk k."""
    from concurrent.futures import ThreadPoolExecutor
    parts = [metas[k:k + chunk] for k in range(0, len(metas), chunk)]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        def submit(j):
            return [pool.submit(read, os.path.join(images_dir, m["file_name"])) for m in parts[j]] if j < len(parts) else []
        files, built = submit(0), []
        for i in range(len(parts) + ahead):         # round i: chunk i is built, chunk i + 1 is read, chunk i - ahead goes out
            if i < len(parts):
                built.append(build(parts[i], files, pool))
            files = submit(i + 1)
            if i >= ahead:
                yield built.pop(0)


# ----------------------------------------------------------------------------- VOC-style AP self-check
def _iou_matrix(det, gt):
    """IoU of every detection [n,4] with every groundtruth box [m,4] (ymin, xmin, ymax, xmax) as metrics.py:234-246
    computes it: 0 unless both the overlap's width and height are positive."""
    w = np.minimum(det[:, None, 3], gt[None, :, 3]) - np.maximum(det[:, None, 1], gt[None, :, 1])
    h = np.minimum(det[:, None, 2], gt[None, :, 2]) - np.maximum(det[:, None, 0], gt[None, :, 0])
    inter = np.where((w > 0) & (h > 0), w * h, 0.0)
    a_d = (det[:, 3] - det[:, 1]) * (det[:, 2] - det[:, 0])
    a_g = (gt[:, 3] - gt[:, 1]) * (gt[:, 2] - gt[:, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (a_d[:, None] + a_g[None, :] - inter)
    return np.where(inter > 0, iou, 0.0)


def average_precision(groundtruth, detections, iou_threshold=0.5):
    """One class.  Semantics of the reference's `evaluate_detector` (metrics.py:156-213):
      groundtruth: {image: float array [m,4]};  detections: list of (image, box[4], confidence).
      * detections are visited in decreasing confidence (stable for ties, like list.sort);
      * a detection's partner is the groundtruth box of its image with the largest IoU (the FIRST such box when IoUs
        tie, `iou > max_iou` in `match`, metrics.py:249-264); it is a true positive iff that IoU >= iou_threshold and the
        box has no earlier partner (a second detection of a matched box is a false positive);
      * precision[k] = TP / (k+1), recall[k] = TP / max(#groundtruth, 1); AP = sum precision[k] * (recall[k] - recall[k-1])
        (metrics.py:274-282); best threshold = the confidence maximising P*R*(1 - |P - R|) (:216-231).
    Returns the reference's seven values."""
    num_gt = max(sum(len(b) for b in groundtruth.values()), 1)
    conf = np.array([d[2] for d in detections], dtype=np.float64)
    order = np.argsort(-conf, kind="stable")
    matched = {img: np.zeros(len(b), bool) for img, b in groundtruth.items()}
    tp = np.zeros(len(detections), bool)
    iou_sum = 0.0
    for k, di in enumerate(order):
        img, box, _c = detections[di]
        gt = groundtruth.get(img)
        if gt is None or len(gt) == 0:
            continue
        iou = _iou_matrix(np.asarray(box, np.float64)[None], np.asarray(gt, np.float64))[0]
        best = int(np.argmax(iou))                      # first maximum, like the strict `>` scan
        if iou[best] > 0 and iou[best] >= iou_threshold and not matched[img][best]:
            matched[img][best] = True
            tp[k] = True
            iou_sum += float(iou[best])
    ctp = np.cumsum(tp)
    n = np.arange(1, len(detections) + 1)
    precision = ctp / np.maximum(n, 1)
    recall = ctp / num_gt
    ap = float(np.sum(precision * np.diff(np.concatenate([[0.0], recall])))) if len(detections) else 0.0
    if len(detections):
        best_i = int(np.argmax(precision * recall * (1.0 - np.abs(precision - recall))))
        best = (float(conf[order][best_i]), float(precision[best_i]), float(recall[best_i]))
    else:
        best = (0.0, 0.0, 0.0)
    ntp = int(ctp[-1]) if len(detections) else 0
    return {"AP": ap, "precision": best[1], "recall": best[2], "best_threshold": best[0],
            "mean_iou_for_TP": iou_sum / max(ntp, 1), "total_FP": len(detections) - ntp, "total_FN": num_gt - ntp}


class Evaluator:
    """Mirror of metrics.py:15-131 without the TF plumbing: detections and groundtruth are kept per label, `evaluate`
    returns the per-label metrics and, for more than one class, their mean AP under the key 'mAP'."""

    def __init__(self, num_classes):
        assert num_classes > 0
        self.num_classes = num_classes
        self.initialize()

    def initialize(self):
        self.detections = {label: [] for label in range(self.num_classes)}
        self.groundtruth = {label: {} for label in range(self.num_classes)}
        self.unique_image_id = 0

    def add_groundtruth(self, image_name, boxes, labels):
        for box, label in zip(np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(labels).reshape(-1)):
            self.groundtruth[int(label)].setdefault(image_name, []).append(box)

    def add_detections(self, image_name, boxes, labels, scores):
        for box, label, score in zip(np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(labels).reshape(-1),
                                     np.asarray(scores).reshape(-1)):
            self.detections[int(label)].append((image_name, box, float(score)))

    def add_image(self, gt_boxes, gt_labels, boxes, labels, scores):
        """One image's groundtruth and the detector's (already num_boxes-trimmed) outputs: `update_op_func`, metrics.py:55-59."""
        name = str(self.unique_image_id)
        self.unique_image_id += 1
        self.add_groundtruth(name, gt_boxes, gt_labels)
        self.add_detections(name, boxes, labels, scores)

    def evaluate(self, iou_threshold=0.5):
        self.metrics = {}
        for label in range(self.num_classes):
            gt = {img: np.array(b, np.float64).reshape(-1, 4) for img, b in self.groundtruth[label].items()}
            self.metrics[label] = average_precision(gt, self.detections[label], iou_threshold)
        if self.num_classes > 1:
            self.metrics["mAP"] = float(np.mean([self.metrics[label]["AP"] for label in range(self.num_classes)]))
        return self.metrics
