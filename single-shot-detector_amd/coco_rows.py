"""The rows of ssd_coco_match straight from the engine's record blocks (include/ssd_hip.h, "the COCO rows"): what
ssd.score_filter + coco_eval.detection_records + CocoBoxEval.__init__ + coco_match.pack make of a run's detections, for all images
at once and without a dict or a tuple per detection.

rows_host() is that function in vectorised numpy -- the CPU path and the kernels' yardstick; rows_device() is ssd_coco_rows_count,
an exclusive scan of the counts and ssd_coco_rows_fill on the current stream, the row arrays left on the GPU; write_predictions()
formats the predictions file's rows from the same flat arrays.  Both row builders raise ValueError for a record the kernels flag."""
import numpy as np

from .coco_match import CELLS_PER_BLOCK, GRID_CAP, MAX_DET      # noqa: F401  (one launch shape for the family)
from .ssd import split_records

# include/ssd_hip.h (tests/test_coco_rows_host.py compares them with the header)
ROWS_MAX_T = 2048
BOX_LIMIT = np.float32(2.0 ** 30)


def _as_records(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != np.int32 or rec.ndim != 2 or rec.shape[1] % 6 != 1 or rec.shape[1] < 7:
        raise ValueError("records must be an int32 block [n_images, 6T + 1]")
    return rec


def _as_hw(image_hw, n):
    hw = np.ascontiguousarray(image_hw, np.int32).reshape(-1, 2)
    if len(hw) != n or (n and hw.min() < 1):
        raise ValueError("image_hw must hold a positive (height, width) for each of the %d records" % n)
    return hw


def _raise_bad(bad, image_ids):
    """bad int32 [n] of include/ssd_hip.h -> ValueError for the first flagged image"""
    at = np.nonzero(bad != -1)[0]
    if len(at):
        i = int(at[0])
        raise ValueError("record row %d of image %r cannot be evaluated: a score or box that is not finite, a label outside the "
                         "mapping, or a num_boxes outside [0, T]" % (int(bad[i]), i if image_ids is None else image_ids[i]))


def _live_rows(rec, hw, thr, num_labels):
    """The kept rows of every record, flat and in (image, row) order -> image index, row, score f32, label, the four float32 products
    [m, 4] (ymin * H, xmin * W, ymax * H, xmax * W), and bad int32 [n] of include/ssd_hip.h."""
    boxes, labels, scores, num = split_records(rec)
    n, T = scores.shape
    bad = np.full(n, -1, np.int32)
    num_ok = (num >= 0) & (num <= T)
    bad[~num_ok] = T
    live = np.arange(T, dtype=np.int64)[None, :] < np.where(num_ok, num, 0).astype(np.int64)[:, None]
    li, lj = np.nonzero(live)
    s, lab = scores[li, lj], labels[li, lj]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(s)
        keep = finite & (s > thr)                                      # float32 > float32, strict
        li, lj, s, lab, dead = li[keep], lj[keep], s[keep], lab[keep], (li[~finite], lj[~finite])
        scaler = hw.astype(np.float32)[:, [0, 1, 0, 1]]
        p = boxes[li, lj] * scaler[li]                                 # four products, each rounded to float32 on its own
        wrong = ~((np.abs(p) < BOX_LIMIT).all(axis=1) & (lab >= 0) & (lab < num_labels))
    first = np.full(n, T, np.int64)
    np.minimum.at(first, dead[0], dead[1])
    np.minimum.at(first, li[wrong], lj[wrong])
    flagged = num_ok & (first < T)
    bad[flagged] = first[flagged]
    ok = ~wrong
    return li[ok], lj[ok], s[ok], lab[ok], p[ok], bad


def _xywh(p):
    """the float32 products [m, 4] -> x, y, w, h int64: truncation toward zero of xmin * W, ymin * H and of the float32 differences"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (p[:, 1].astype(np.int64), p[:, 0].astype(np.int64), (p[:, 3] - p[:, 1]).astype(np.int64), (p[:, 2] - p[:, 0]).astype(np.int64))


def rows_host(records, image_hw, label_to_cat, K, score_threshold, image_ids=None):
    """records int32 [n, 6T + 1] (numpy), image_hw [n, 2] (height, width of the original images), label_to_cat int [num_labels] (index
    into cat_ids or -1) -> {'counts' int32 [K, n], 'det_box' float64 [nd, 4] xywh, 'det_area' [nd], 'det_score' [nd]}: the rows of
    include/ssd_hip.h, "the COCO rows", cell after cell in the order of the flattened counts -- one lexsort, no per-row Python.
    ValueError naming the image (image_ids[i], else its position) and the record row for a record the header calls bad."""
    rec = _as_records(records)
    n = len(rec)
    hw = _as_hw(image_hw, n)
    l2c = np.ascontiguousarray(label_to_cat, np.int64).reshape(-1)
    K = int(K)
    li, lj, s, lab, p, bad = _live_rows(rec, hw, np.float32(score_threshold), len(l2c))
    _raise_bad(bad, image_ids)
    k = l2c[lab]
    ok = (k >= 0) & (k < K)
    li, lj, s, p, k = li[ok], lj[ok], s[ok], p[ok], k[ok]
    order = np.lexsort((lj, -s, li, k))                    # category, image, descending score, ascending record row
    cell = (k * n + li)[order]
    full = np.bincount(cell, minlength=K * n).astype(np.int64)
    rank = np.arange(len(order), dtype=np.int64) - (np.cumsum(full) - full)[cell]
    order = order[rank < MAX_DET]
    x, y, w, h = _xywh(p[order])
    return {"counts": np.minimum(full, MAX_DET).astype(np.int32).reshape(K, n),
            "det_box": np.ascontiguousarray(np.stack([x, y, w, h], axis=1).astype(np.float64)).reshape(-1, 4),
            "det_area": (w * h).astype(np.float64), "det_score": s[order].astype(np.float64)}


def launch_count(records, image_hw, label_to_cat, K, score_threshold, counts, bad):
    """ssd_coco_rows_count on the current stream of the tensors' device: records int32 [n, 6T + 1], image_hw int32 [n, 2],
    label_to_cat int32 [num_labels], counts int32 [K, n], bad int32 [n] -- torch tensors on one GPU."""
    import torch
    from ._lib import check, lib
    from .metric_calls import stream
    n, words = records.shape
    with torch.cuda.device(records.device):
        check(lib().ssd_coco_rows_count(records.data_ptr(), n, (words - 1) // 6, image_hw.data_ptr(), label_to_cat.data_ptr(),
                                        label_to_cat.numel(), int(K), float(score_threshold), counts.data_ptr(), bad.data_ptr(),
                                        stream(records.device)))


def launch_fill(records, image_hw, label_to_cat, K, score_threshold, det_begin, nd, det_box, det_area, det_score):
    """ssd_coco_rows_fill on the current stream of the tensors' device: det_begin int64 [K, n], the three row arrays float64 [nd, 4] /
    [nd] / [nd] (any dtype that holds the bytes)."""
    import torch
    from ._lib import check, lib
    from .metric_calls import stream
    n, words = records.shape
    with torch.cuda.device(records.device):
        check(lib().ssd_coco_rows_fill(records.data_ptr(), n, (words - 1) // 6, image_hw.data_ptr(), label_to_cat.data_ptr(),
                                       label_to_cat.numel(), int(K), float(score_threshold), det_begin.data_ptr(), int(nd),
                                       det_box.data_ptr(), det_area.data_ptr(), det_score.data_ptr(), stream(records.device)))


def rows_device(records, image_hw, label_to_cat, K, score_threshold, device, image_ids=None, timings=None):
    """rows_host() on `device` (a CUDA device index or torch.device): records a torch tensor on that GPU or a numpy block (uploaded).
    count, the exclusive scan of the flattened counts (torch.cumsum on the device), fill -- on the current stream.
    -> {'counts' int32 [K, n] and 'det_score' float64 [nd] on the host, 'det_box' [nd, 4], 'det_area' [nd] torch float64 tensors on
    the GPU}; only counts, bad and det_score are downloaded.  timings: a dict that receives 'count', 'scan', 'fill' (HIP events) and
    'download' in seconds."""
    import time
    import torch
    from . import metric_calls
    dev = metric_calls.device_of(device)
    up, tm = metric_calls.uploader(dev, "the records", contiguous=True), metric_calls.Timer(dev, timings is not None)
    K = int(K)
    with torch.cuda.device(dev):
        rec = up(records if isinstance(records, torch.Tensor) else _as_records(records))
        if rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] % 6 != 1 or rec.shape[1] < 7:
            raise ValueError("records must be an int32 block [n_images, 6T + 1]")
        n = rec.shape[0]
        hw = up(_as_hw(image_hw, n))
        l2c = up(np.ascontiguousarray(label_to_cat, np.int32).reshape(-1))
        counts = torch.empty((K, n), dtype=torch.int32, device=dev)
        bad = torch.empty((n,), dtype=torch.int32, device=dev)
        e0 = tm.mark()
        launch_count(rec, hw, l2c, K, score_threshold, counts, bad)
        e1 = tm.mark()
        t0 = time.perf_counter()
        counts_host, bad_host = counts.cpu().numpy(), bad.cpu().numpy()
        t1 = time.perf_counter()
        _raise_bad(bad_host, image_ids)
        nd = int(counts_host.sum(dtype=np.int64))
        e2 = tm.mark()
        flat = counts.view(-1)
        det_begin = torch.cumsum(flat, 0, dtype=torch.int64) - flat
        e3 = tm.mark()
        det_box = torch.empty((nd, 4), dtype=torch.float64, device=dev)
        det_area = torch.empty((nd,), dtype=torch.float64, device=dev)
        det_score = torch.empty((nd,), dtype=torch.float64, device=dev)
        e4 = tm.mark()
        launch_fill(rec, hw, l2c, K, score_threshold, det_begin, nd, det_box, det_area, det_score)
        e5 = tm.mark()
        t2 = time.perf_counter()
        score_host = det_score.cpu().numpy()
        if timings is not None:
            t3 = time.perf_counter()
            timings.update(count=tm.seconds(e0, e1), scan=tm.seconds(e2, e3), fill=tm.seconds(e4, e5), download=(t1 - t0) + (t3 - t2))
    return {"counts": counts_host, "det_box": det_box, "det_area": det_area, "det_score": score_host}


_ROW = '{{"image_id": {}, "category_id": {}, "bbox": [{}, {}, {}, {}], "score": {}}}'.format


def write_predictions(records_host, image_ids, image_hw, label_to_coco_id, score_threshold):
    """The predictions file's rows of these images as bytes: json.dumps(coco_eval.detection_records_many(...))[1:-1], byte for byte
    (rows in image order, inside an image in record order; `, ` / `: ` separators; the score is repr of the widened float32),
    formatted from flat arrays -- no dict is built.  label_to_coco_id: {detector label: official category id}."""
    rec = _as_records(records_host)
    hw = _as_hw(image_hw, len(rec))
    ids = [int(i) for i in image_ids]
    if len(ids) != len(rec):
        raise ValueError("%d image ids for %d records" % (len(ids), len(rec)))
    num_labels = max(label_to_coco_id) + 1 if label_to_coco_id else 1
    coco_id = np.full(num_labels, -1, np.int64)
    for label, cat in label_to_coco_id.items():
        coco_id[int(label)] = int(cat)
    li, lj, s, lab, p, bad = _live_rows(rec, hw, np.float32(score_threshold), num_labels)
    _raise_bad(bad, ids)
    cat = coco_id[lab]
    if (cat < 0).any():
        raise ValueError("label %d has no category id" % int(lab[np.nonzero(cat < 0)[0][0]]))
    x, y, w, h = _xywh(p)
    scores = map(repr, s.astype(np.float64).tolist())
    return ", ".join(map(_ROW, np.asarray(ids, object)[li].tolist(), cat.tolist(), x.tolist(), y.tolist(), w.tolist(), h.tolist(),
                         scores)).encode()
