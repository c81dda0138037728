"""The GPU path of CocoBoxEval.evaluate (include/ssd_hip.h, "the COCO box matching"): the cells of a run packed
into flat arrays, one ssd_coco_match launch, the packed bits unpacked into the tuples the host loop makes.

pack() needs numpy alone (the host tests call it); match() uploads, launches on the current stream and downloads; match_device()
leaves the outputs on the GPU, where ssd_coco_accumulate reads them (coco_accumulate.py)."""
import ctypes

import numpy as np

# include/ssd_hip.h (tests/test_coco_match_host.py compares them with the header)
MAX_DET = 100
MAX_GT = 256
MAX_THR = 16
MAX_AREA = 4
CELLS_PER_BLOCK = 4
GRID_CAP = 1024
CELL_DTYPE = np.dtype([("det_begin", "<i8"), ("gt_begin", "<i8"), ("D", "<i4"), ("G", "<i4")])
assert CELL_DTYPE.itemsize == 24


def _finite(values, what, owner):
    """owner(k) -> (image id, category id, position in that cell's input) of row k"""
    if not len(values):
        return
    bad = np.nonzero(~np.isfinite(values).reshape(len(values), -1).all(axis=1))[0]
    if len(bad):
        img, cat, pos = owner(int(bad[0]))
        raise ValueError("%s %d of image %r, category %r is not finite" % (what, pos, img, cat))


def pack(gts, dts, cat_ids, subset):
    """The cells of the images `subset` (ascending) in the host loop's order -- category ascending, image ascending -- as the
    flat arrays of include/ssd_hip.h.  gts / dts: CocoBoxEval's {(image, category): [(bbox, area, crowd)]} /
    {(image, category): [(bbox, area, score)]}.  Detections are ordered and truncated by ONE stable sort over all rows, keyed by
    (cell, -score).  Cells with more than MAX_GT groundtruth boxes are not packed (packed[k] False): the host loop computes them.

    -> dict: keys [(category, image)] of every cell, packed and fallback, in order; packed bool [len(keys)]; cells CELL_DTYPE [n];
       det_box [nd,4], det_area [nd], det_score [nd] float64; gt_box [ng,4], gt_area [ng] float64, gt_crowd [ng] uint8"""
    want = set(subset)
    cats = set(cat_ids)
    present = set(k for k in gts if gts[k]) | set(k for k in dts if dts[k])
    keys = sorted((cat, img) for img, cat in present if img in want and cat in cats)
    packed = np.array([len(gts.get((img, cat), ())) <= MAX_GT for cat, img in keys], bool).reshape(-1)
    mine = [k for k, p in zip(keys, packed.tolist()) if p]
    det_rows, gt_rows, n_det, n_gt = [], [], [], []
    for cat, img in mine:
        d, g = dts.get((img, cat), ()), gts.get((img, cat), ())
        det_rows += d
        gt_rows += g
        n_det.append(len(d))
        n_gt.append(len(g))
    n_det, n_gt = np.array(n_det, np.int64).reshape(-1), np.array(n_gt, np.int64).reshape(-1)
    det_first = np.concatenate([[0], np.cumsum(n_det)]).astype(np.int64)
    gt_first = np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int64)

    def owner(first):
        def of(k):
            c = int(np.searchsorted(first, k, side="right")) - 1
            return mine[c][1], mine[c][0], k - int(first[c])
        return of
    box = np.array([r[0] for r in det_rows], np.float64).reshape(-1, 4)
    area = np.array([r[1] for r in det_rows], np.float64).reshape(-1)
    score = np.array([r[2] for r in det_rows], np.float64).reshape(-1)
    _finite(box, "the box of detection", owner(det_first))
    _finite(area, "the area of detection", owner(det_first))
    _finite(score, "the score of detection", owner(det_first))
    gt_box = np.array([r[0] for r in gt_rows], np.float64).reshape(-1, 4)
    gt_area = np.array([r[1] for r in gt_rows], np.float64).reshape(-1)
    gt_crowd = (np.array([r[2] for r in gt_rows], np.int64).reshape(-1) != 0).astype(np.uint8)
    _finite(gt_box, "the box of groundtruth box", owner(gt_first))
    _finite(gt_area, "the area of groundtruth box", owner(gt_first))
    # one stable sort: by cell, inside a cell by descending score, ties in input order; then the first MAX_DET of every cell
    cell_of = np.repeat(np.arange(len(mine), dtype=np.int64), n_det)
    order = np.lexsort((-score, cell_of))
    rank = np.arange(len(order), dtype=np.int64) - det_first[cell_of]       # (cell_of is sorted: order keeps the cells' blocks)
    order = order[rank < MAX_DET]
    cells = np.zeros(len(mine), CELL_DTYPE)
    cells["D"] = np.minimum(n_det, MAX_DET)
    cells["G"] = n_gt
    cells["det_begin"] = np.cumsum(cells["D"], dtype=np.int64) - cells["D"]
    cells["gt_begin"] = gt_first[:-1]
    return {"keys": keys, "packed": packed, "cells": cells,
            "det_box": np.ascontiguousarray(box[order]), "det_area": np.ascontiguousarray(area[order]),
            "det_score": np.ascontiguousarray(score[order]), "gt_box": gt_box, "gt_area": gt_area, "gt_crowd": gt_crowd}


def launch(cells_host, cells_dev, det_box, det_area, nd, gt_box, gt_area, gt_crowd, ng, thr, area_rng, matched, ignored, gt_ignore, iou=None):
    """ssd_coco_match on the current stream of the tensors' device.  cells_host: CELL_DTYPE array; every other array a torch tensor
    on one GPU, of any dtype that holds the bytes: cells_dev [n * 24 bytes], float64 boxes [nd, 4] / [ng, 4] and areas [nd] / [ng],
    uint8 crowd [ng], matched / ignored [A, nd] uint16 words, gt_ignore uint8 [A, ng], iou float64 [sum D * G] or None.
    thr [T], area_rng [A, 2]: float64 values on the host."""
    import torch
    from ._lib import check, lib
    from .metric_calls import stream
    thr = np.ascontiguousarray(thr, np.float64).reshape(-1)
    rng = np.ascontiguousarray(area_rng, np.float64).reshape(-1, 2)
    cells_host = np.ascontiguousarray(cells_host, CELL_DTYPE)
    dev = matched.device
    dp = ctypes.POINTER(ctypes.c_double)
    with torch.cuda.device(dev):
        check(lib().ssd_coco_match(cells_host.ctypes.data, cells_dev.data_ptr(), len(cells_host), det_box.data_ptr(), det_area.data_ptr(),
                                   int(nd), gt_box.data_ptr(), gt_area.data_ptr(), gt_crowd.data_ptr(), int(ng),
                                   thr.ctypes.data_as(dp), len(thr), rng.ctypes.data_as(dp), len(rng), matched.data_ptr(),
                                   ignored.data_ptr(), gt_ignore.data_ptr(), None if iou is None else iou.data_ptr(),
                                   stream(dev)))


def match_device(p, thr, area_rng, device, want_iou=False, timings=None):
    """pack()'s arrays (det_box / det_area numpy, or torch tensors already on `device`) through the kernel, the outputs left on the GPU -> matched, ignored torch uint8 [A, nd, 2] (the uint16 words'
    bytes), gt_ignore torch uint8 [A, ng], the IoU dump float64 [sum D * G] or None.  The launch is enqueued on the current stream;
    nothing waits for it unless timings is given: a dict that receives 'upload' and 'launch' (HIP events) in seconds."""
    import time
    import torch
    from . import metric_calls
    dev = metric_calls.device_of(device)
    up = metric_calls.uploader(dev, "the detections' rows", contiguous=True)    # (tensors: the rows coco_rows.rows_device left on this GPU)
    tm = metric_calls.Timer(dev, timings is not None)
    A = len(area_rng)
    nd, ng = len(p["det_area"]), len(p["gt_area"])
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        cells_dev = up(p["cells"], as_bytes=True)
        det_box, det_area = up(p["det_box"]), up(p["det_area"])
        gt_box, gt_area, gt_crowd = up(p["gt_box"]), up(p["gt_area"]), up(p["gt_crowd"])
        matched = torch.empty((A, nd, 2), dtype=torch.uint8, device=dev)
        ignored = torch.empty((A, nd, 2), dtype=torch.uint8, device=dev)
        gt_ignore = torch.empty((A, ng), dtype=torch.uint8, device=dev)
        iou = torch.empty(int((p["cells"]["D"].astype(np.int64) * p["cells"]["G"]).sum()), dtype=torch.float64, device=dev) if want_iou else None
        t1, e0 = tm.uploaded(), tm.mark()
        launch(p["cells"], cells_dev, det_box, det_area, nd, gt_box, gt_area, gt_crowd, ng, thr, area_rng, matched, ignored, gt_ignore, iou)
        if timings is not None:
            timings.update(upload=t1 - t0, launch=tm.seconds(e0, tm.mark()))
    return matched, ignored, gt_ignore, iou


def download_words(matched, ignored, gt_ignore):
    """match_device()'s tensors on the host -> matched, ignored uint16 [A, nd] (bit t), gt_ignore uint8 [A, ng]"""
    A, nd = matched.shape[0], matched.shape[1]
    m = matched.cpu().numpy().view(np.uint16).reshape(A, nd)
    i = ignored.cpu().numpy().view(np.uint16).reshape(A, nd)
    return m, i, gt_ignore.cpu().numpy()


def match(p, thr, area_rng, device, want_iou=False, timings=None):
    """pack()'s arrays through the kernel -> matched, ignored bool [A, T, nd], gt_ignore bool [A, ng] (and the IoU dump float64
    [sum D * G] with want_iou).  timings: a dict that receives 'upload', 'launch' (HIP events) and 'download' in seconds."""
    import time
    matched, ignored, gt_ignore, iou = match_device(p, thr, area_rng, device, want_iou, timings)
    t2 = time.perf_counter()
    m, i, g = download_words(matched, ignored, gt_ignore)
    dump = iou.cpu().numpy() if want_iou else None
    if timings is not None:
        timings.update(download=time.perf_counter() - t2)
    out = unpack_bits(m, len(thr)), unpack_bits(i, len(thr)), g.astype(bool)
    return out + (dump,) if want_iou else out


def unpack_bits(words, T):
    """uint16 [A, nd], bit t -> bool [A, T, nd]"""
    shifts = np.arange(T, dtype=np.uint16).reshape(1, T, 1)
    return ((words[:, None, :] >> shifts) & np.uint16(1)).astype(bool)
