"""The GPU path of coco_eval.Evaluator.evaluate (include/ssd_hip.h, "the VOC-style metric"): the detections of a
run sorted once into the global order, their (label, image) cells packed into flat arrays, one ssd_voc_match and one ssd_voc_curve
launch, n_labels x 64 bytes downloaded and turned into the dict Evaluator.evaluate returns.

pack() and scan_cell() need numpy alone (the host tests call them); evaluate_packed() uploads, launches on the current stream and
downloads."""
import numpy as np

# include/ssd_hip.h (tests/test_voc_match_host.py compares them with the header)
MAX_GT = 4096
CELLS_PER_BLOCK = 4
GRID_CAP = 1024
CELL_DTYPE = np.dtype([("det_begin", "<i8"), ("gt_begin", "<i8"), ("D", "<i4"), ("G", "<i4")])
SEGMENT_DTYPE = np.dtype([("begin", "<i8"), ("count", "<i8"), ("num_gt", "<i8")])
RESULT_DTYPE = np.dtype([("ap", "<f8"), ("precision", "<f8"), ("recall", "<f8"), ("best_threshold", "<f8"), ("mean_iou", "<f8"),
                         ("tp", "<i8"), ("best_index", "<i8"), ("reserved", "<i8")])
assert CELL_DTYPE.itemsize == 24 and SEGMENT_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 64


def scan_cell(det_box, gt_box, thr):
    """The scan of one cell on the host (the header's rule through coco_eval._iou_matrix): det_box [D,4] in global order, gt_box
    [G,4] in insertion order -> tp uint8 [D], tp_iou float64 [D].  evaluate_packed() places the cells over MAX_GT with it."""
    from .coco_eval import _iou_matrix
    det_box, gt_box = np.asarray(det_box, np.float64).reshape(-1, 4), np.asarray(gt_box, np.float64).reshape(-1, 4)
    tp, tp_iou = np.zeros(len(det_box), np.uint8), np.zeros(len(det_box), np.float64)
    taken = np.zeros(len(gt_box), bool)
    if len(gt_box):
        for d in range(len(det_box)):
            iou = _iou_matrix(det_box[d:d + 1], gt_box)[0]
            best = int(np.argmax(iou))
            if iou[best] > 0 and iou[best] >= thr and not taken[best]:
                taken[best] = True
                tp[d], tp_iou[d] = 1, iou[best]
    return tp, tp_iou


def pack(num_classes, n_images, gt_box, gt_label, gt_image, det_box, det_label, det_image, det_conf):
    """The rows of a run as the flat arrays of include/ssd_hip.h.  gt_* / det_*: every groundtruth box / detection of the run in
    insertion order -- float64 boxes [n,4] (ymin, xmin, ymax, xmax), int64 labels in [0, num_classes) and images in [0, n_images),
    float64 confidences, all finite.  Two np.lexsorts order the detections: (label, -confidence), stable, is the global order;
    (label, image) over that, stable, is the cell order.  A cell with more than MAX_GT groundtruth boxes is not packed: its rows
    come back under 'fallback' for scan_cell().

    -> dict: n_rows; order int64 [n_rows] (row pos is detection order[pos]); conf float64 [n_rows] in global order; segments
       SEGMENT_DTYPE [num_classes]; cells CELL_DTYPE [n]; det_box float64 [nd,4] and det_pos int32 [nd] in cell order; gt_box
       float64 [ng,4], every box of the run by (label, image), insertion order inside; fallback [(pos int64 [D], det_box [D,4],
       gt_box [G,4])]"""
    gt_box, det_box = np.asarray(gt_box, np.float64).reshape(-1, 4), np.asarray(det_box, np.float64).reshape(-1, 4)
    gt_label, gt_image = np.asarray(gt_label, np.int64).reshape(-1), np.asarray(gt_image, np.int64).reshape(-1)
    det_label, det_image = np.asarray(det_label, np.int64).reshape(-1), np.asarray(det_image, np.int64).reshape(-1)
    det_conf = np.asarray(det_conf, np.float64).reshape(-1)
    n_rows = len(det_conf)
    if n_rows > 2 ** 31 - 1:
        raise ValueError("%d detections: det_pos is int32" % n_rows)
    order = np.lexsort((-det_conf, det_label))                         # stable: ties in insertion order
    label, image = det_label[order], det_image[order]
    count = np.bincount(det_label, minlength=num_classes).astype(np.int64)
    segments = np.zeros(num_classes, SEGMENT_DTYPE)
    segments["count"] = count
    segments["begin"] = np.cumsum(count) - count
    segments["num_gt"] = np.maximum(np.bincount(gt_label, minlength=num_classes), 1)
    # groundtruth by (label, image): one stable sort of one key
    gt_key = gt_label * n_images + gt_image
    gt_order = np.argsort(gt_key, kind="stable")
    gt_cells, gt_first, gt_count = np.unique(gt_key[gt_order], return_index=True, return_counts=True)
    # the cells: runs of one (label, image) in the cell order
    pos = np.lexsort((image, label))                                    # stable: pos ascends inside a cell
    key = label[pos] * n_images + image[pos]
    first = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if n_rows else np.zeros(0, np.int64)
    D = np.diff(np.concatenate([first, [n_rows]]))
    # a cell's boxes: the run of its key among the sorted boxes; without one, G = 0 at the place the run would have (gt_begin ascends)
    at = np.searchsorted(gt_cells, key[first])
    has = np.concatenate([gt_cells, [-1]])[at] == key[first]
    G = np.where(has, np.concatenate([gt_count, [0]])[at], 0).astype(np.int64)
    g0 = np.concatenate([gt_first, [len(gt_key)]])[at].astype(np.int64)
    sorted_gt = np.ascontiguousarray(gt_box[gt_order])
    fallback = []
    keep = G <= MAX_GT
    for c in np.nonzero(~keep)[0].tolist():
        rows = pos[first[c]:first[c] + D[c]]
        fallback.append((rows, det_box[order[rows]], sorted_gt[g0[c]:g0[c] + G[c]]))
    if not keep.all():
        pos = pos[np.repeat(keep, D)]
        D, G, g0 = D[keep], G[keep], g0[keep]
    cells = np.zeros(len(D), CELL_DTYPE)
    cells["D"], cells["G"], cells["gt_begin"] = D, G, g0
    cells["det_begin"] = np.cumsum(D) - D
    return {"n_rows": n_rows, "order": order, "conf": np.ascontiguousarray(det_conf[order]), "segments": segments, "cells": cells,
            "det_box": np.ascontiguousarray(det_box[order[pos]]), "det_pos": pos.astype(np.int32), "gt_box": sorted_gt,
            "fallback": fallback}


def launch(cells_host, cells_dev, det_box, det_pos, nd, gt_box, ng, thr, tp, tp_iou, n_rows, segments_host=None, segments_dev=None,
           conf=None, results=None):
    """ssd_voc_match and, with segments, ssd_voc_curve behind it on the current stream of the tensors' device.  cells_host /
    segments_host: CELL_DTYPE / SEGMENT_DTYPE arrays; every other array a torch tensor on one GPU, of any dtype that holds the bytes:
    cells_dev [n * 24 bytes], float64 boxes [nd,4] / [ng,4], det_pos int32 [nd], tp uint8 [n_rows], tp_iou and conf float64 [n_rows],
    segments_dev [L * 24 bytes], results [L * 64 bytes].  cells_host None: the curve alone."""
    import torch
    from ._lib import check, lib
    from . import metric_calls
    dev = tp.device
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        stream = metric_calls.stream(dev)                                   # both calls on one stream
        if cells_host is not None:
            cells_host = np.ascontiguousarray(cells_host, CELL_DTYPE)
            check(lib().ssd_voc_match(cells_host.ctypes.data, ptr(cells_dev), len(cells_host), ptr(det_box), ptr(det_pos), int(nd), ptr(gt_box),
                                      int(ng), float(thr), ptr(tp), ptr(tp_iou), int(n_rows), stream))
        if segments_host is not None:
            segments_host = np.ascontiguousarray(segments_host, SEGMENT_DTYPE)
            check(lib().ssd_voc_curve(segments_host.ctypes.data, ptr(segments_dev), len(segments_host), ptr(tp), ptr(tp_iou), ptr(conf),
                                      int(n_rows), ptr(results), stream))


def evaluate_packed(p, thr, device, want_rows=False, timings=None):
    """pack()'s arrays through the two kernels -> results RESULT_DTYPE [num_classes] (and with want_rows: tp uint8 [n_rows], tp_iou
    float64 [n_rows] in global order).  The cells under 'fallback' are scanned on the host and travel inside the output buffers, at
    rows the match kernel never writes.  timings: a dict that receives 'upload', 'match', 'curve' (HIP events), 'download' in seconds."""
    import time
    import torch
    from . import metric_calls
    if not np.isfinite(thr):
        raise ValueError("iou_threshold %r is not finite" % (thr,))
    dev = metric_calls.device_of(device)
    up, tm = metric_calls.uploader(dev), metric_calls.Timer(dev, timings is not None)
    n_rows, nd, ng, L = p["n_rows"], len(p["det_pos"]), len(p["gt_box"]), len(p["segments"])
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        cells_dev, segments_dev = up(p["cells"], as_bytes=True), up(p["segments"], as_bytes=True)
        det_box, det_pos, gt_box, conf = up(p["det_box"]), up(p["det_pos"]), up(p["gt_box"]), up(p["conf"])
        if p["fallback"]:
            tp_host, iou_host = np.zeros(n_rows, np.uint8), np.zeros(n_rows, np.float64)
            for rows, dbox, gbox in p["fallback"]:
                tp_host[rows], iou_host[rows] = scan_cell(dbox, gbox, thr)
            tp, tp_iou = up(tp_host), up(iou_host)
        else:
            tp = torch.empty(n_rows, dtype=torch.uint8, device=dev)
            tp_iou = torch.empty(n_rows, dtype=torch.float64, device=dev)
        results = torch.empty(L * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        t1, e0 = tm.uploaded(), tm.mark()
        launch(p["cells"], cells_dev, det_box, det_pos, nd, gt_box, ng, thr, tp, tp_iou, n_rows)
        e1 = tm.mark()
        launch(None, None, None, None, 0, None, 0, thr, tp, tp_iou, n_rows, p["segments"], segments_dev, conf, results)
        curve, match = tm.seconds(e1, tm.mark()), tm.seconds(e0, e1)
        t2 = time.perf_counter()
        out = results.cpu().numpy().view(RESULT_DTYPE)
        rows = (tp.cpu().numpy(), tp_iou.cpu().numpy()) if want_rows else None
        if timings is not None:
            timings.update(upload=t1 - t0, match=match, curve=curve, download=time.perf_counter() - t2)
    return (out,) + rows if want_rows else out


def metrics_dict(p, results):
    """results RESULT_DTYPE [num_classes] -> the dict of Evaluator.evaluate: per label the seven values, 'mAP' for more than one class"""
    seg = p["segments"]
    m = {}
    for label, (r, n, num_gt) in enumerate(zip(results.tolist(), seg["count"].tolist(), seg["num_gt"].tolist())):
        ap, precision, recall, best_threshold, mean_iou, tp = r[:6]
        m[label] = {"AP": ap, "precision": precision, "recall": recall, "best_threshold": best_threshold, "mean_iou_for_TP": mean_iou,
                    "total_FP": n - tp, "total_FN": num_gt - tp}
    if len(seg) > 1:
        m["mAP"] = float(np.mean([m[label]["AP"] for label in range(len(seg))]))
    return m


class VocEvaluator:
    """coco_eval.Evaluator with the images kept as arrays: add_image stores its five arrays as they come (one append per image, no
    Python per box); evaluate(device=None) feeds them to an Evaluator and returns its dict unchanged, evaluate(device=d) computes the
    same dict on GPU d -- every value bit for bit, except 'AP' (and their mean 'mAP'), which the kernel sums in row order where the
    host's np.sum adds pairwise: equal within 2 * tp * 2^-53."""

    def __init__(self, num_classes):
        assert num_classes > 0
        self.num_classes = num_classes
        self.initialize()

    def initialize(self):
        self.images = []                                                # (gt_boxes, gt_labels, boxes, labels, scores) per image
        self.unique_image_id = 0

    def add_image(self, gt_boxes, gt_labels, boxes, labels, scores):
        gt_boxes, boxes = np.array(gt_boxes, np.float64).reshape(-1, 4), np.array(boxes, np.float64).reshape(-1, 4)
        gt_labels, labels = np.array(gt_labels).reshape(-1).astype(np.int64), np.array(labels).reshape(-1).astype(np.int64)
        scores = np.array(scores).reshape(-1).astype(np.float64)
        if len(gt_labels) != len(gt_boxes) or len(labels) != len(boxes) or len(scores) != len(boxes):
            raise ValueError("image %d: %d groundtruth boxes with %d labels, %d boxes with %d labels and %d scores"
                             % (self.unique_image_id, len(gt_boxes), len(gt_labels), len(boxes), len(labels), len(scores)))
        for what, lab in (("groundtruth", gt_labels), ("detection", labels)):
            bad = np.nonzero((lab < 0) | (lab >= self.num_classes))[0]
            if len(bad):                                                # Evaluator: the lookup of self.groundtruth[label] fails
                raise KeyError("image %d: %s label %d (row %d) is outside [0, %d)"
                               % (self.unique_image_id, what, int(lab[bad[0]]), int(bad[0]), self.num_classes))
        self.images.append((gt_boxes, gt_labels, boxes, labels, scores))
        self.unique_image_id += 1

    def _flat(self):
        """-> pack()'s arguments behind num_classes, every value checked to be finite"""
        cat = lambda i, shape, dtype: (np.concatenate([im[i] for im in self.images]) if self.images else np.zeros(shape, dtype))
        gt_box, gt_label = cat(0, (0, 4), np.float64), cat(1, (0,), np.int64)
        det_box, det_label, det_conf = cat(2, (0, 4), np.float64), cat(3, (0,), np.int64), cat(4, (0,), np.float64)
        ids = np.arange(len(self.images), dtype=np.int64)
        gt_image = np.repeat(ids, [len(im[1]) for im in self.images])
        det_image = np.repeat(ids, [len(im[3]) for im in self.images])
        for what, values, owner in (("groundtruth box", gt_box, gt_image), ("box of detection", det_box, det_image),
                                    ("score of detection", det_conf, det_image)):
            bad = np.nonzero(~np.isfinite(values).reshape(len(values), 4 if values.ndim > 1 else 1).all(axis=1))[0]
            if len(bad):
                img = int(owner[bad[0]])
                raise ValueError("the %s %d of image %d is not finite" % (what, int(bad[0]) - int(np.searchsorted(owner, img)), img))
        return len(self.images), gt_box, gt_label, gt_image, det_box, det_label, det_image, det_conf

    def evaluate(self, iou_threshold=0.5, device=None, timings=None):
        """timings (device=d only): a dict that receives 'pack', evaluate_packed's parts and 'dict' in seconds."""
        import time
        if device is None:
            from .coco_eval import Evaluator
            ev = Evaluator(self.num_classes)
            for im in self.images:
                ev.add_image(*im)
            self.metrics = ev.evaluate(iou_threshold)
            return self.metrics
        if not np.isfinite(iou_threshold):
            raise ValueError("iou_threshold %r is not finite" % (iou_threshold,))
        t0 = time.perf_counter()
        p = pack(self.num_classes, *self._flat())
        t1 = time.perf_counter()
        results = evaluate_packed(p, float(iou_threshold), device, timings=timings)
        t2 = time.perf_counter()
        self.metrics = metrics_dict(p, results)
        if timings is not None:
            timings.update(pack=t1 - t0, dict=time.perf_counter() - t2)
        return self.metrics
