"""The GPU path of CocoBoxEval.accumulate (include/ssd_hip.h, "the COCO accumulation"): the global order of the
packed detections from one np.lexsort, one ssd_coco_accumulate launch over the matching's outputs, precision and recall read back.

pack_order() and pack_cells() need numpy alone (the host tests call them); accumulate() uploads what is not on the GPU yet, launches
on the current stream and downloads the two arrays."""
import ctypes

import numpy as np

from .coco_match import CELLS_PER_BLOCK, GRID_CAP, MAX_AREA, MAX_DET, MAX_THR      # noqa: F401  (one launch shape for both kernels)

# include/ssd_hip.h (tests/test_coco_accumulate_host.py compares them with the header)
MAX_MAXDETS = 4
MAX_REC = 128
SEGMENT_DTYPE = np.dtype([("det_begin", "<i8"), ("det_count", "<i8"), ("gt_begin", "<i8"), ("gt_count", "<i8")])
assert SEGMENT_DTYPE.itemsize == 32


def _ranges(start, n):
    """the concatenation of arange(start[i], start[i] + n[i])"""
    n = np.asarray(n, np.int64)
    first = np.cumsum(n) - n
    return np.repeat(np.asarray(start, np.int64) - first, n) + np.arange(int(n.sum()), dtype=np.int64)


def _order(cell_cat, D, G, score, K):
    """Cells in packed order (category index ascending, image ascending) with D rows and G groundtruth boxes each, score float64
    [sum D] -> {'order' int32 [nd], 'rank' uint8 [nd], 'segments' SEGMENT_DTYPE [K], 'nd', 'ng'} of include/ssd_hip.h."""
    cell_cat, D, G = np.asarray(cell_cat, np.int64).reshape(-1), np.asarray(D, np.int64).reshape(-1), np.asarray(G, np.int64).reshape(-1)
    score = np.asarray(score, np.float64).reshape(-1)
    nd, ng = int(D.sum()), int(G.sum())
    if nd != len(score) or nd > 2 ** 31 - 1:
        raise ValueError("%d detection rows for %d scores (order is int32: at most 2^31 - 1)" % (nd, len(score)))
    if len(cell_cat) and ((np.diff(cell_cat) < 0).any() or cell_cat[0] < 0 or cell_cat[-1] >= K):
        raise ValueError("the cells must come category-major, in cat_ids order")
    if len(D) and D.max() > MAX_DET:
        raise ValueError("a cell holds %d detections: at most %d" % (int(D.max()), MAX_DET))
    cell_of = np.repeat(np.arange(len(D), dtype=np.int64), D)
    rank = (np.arange(nd, dtype=np.int64) - (np.cumsum(D) - D)[cell_of]).astype(np.uint8)
    # ONE stable sort: category, then descending score, ties by ascending packed row (the host's mergesort over the concatenation)
    order = np.lexsort((-score, cell_cat[cell_of])).astype(np.int32)
    segments = np.zeros(K, SEGMENT_DTYPE)
    np.add.at(segments["det_count"], cell_cat, D)
    np.add.at(segments["gt_count"], cell_cat, G)
    segments["det_begin"] = np.cumsum(segments["det_count"]) - segments["det_count"]
    segments["gt_begin"] = np.cumsum(segments["gt_count"]) - segments["gt_count"]
    return {"order": order, "rank": rank, "segments": segments, "nd": nd, "ng": ng}


def pack_order(p, cat_ids):
    """coco_match.pack()'s dict (every cell packed or not: only the packed ones have rows) -> the row inputs and the segments of
    ssd_coco_accumulate for the categories `cat_ids` (ascending, as CocoBoxEval keeps them)."""
    index = {c: k for k, c in enumerate(cat_ids)}
    cell_cat = [index[cat] for (cat, _img), packed in zip(p["keys"], p["packed"].tolist()) if packed]
    return _order(cell_cat, p["cells"]["D"], p["cells"]["G"], p["det_score"], len(cat_ids))


def words(bits):
    """bool [T, n] -> uint16 [n], bit t (the inverse of coco_match.unpack_bits for one area range)"""
    T = bits.shape[0]
    if T > MAX_THR:
        raise ValueError("%d thresholds: at most %d bits in a word" % (T, MAX_THR))
    out = np.zeros(bits.shape[1], np.uint16)
    for t in range(T):
        out |= bits[t].astype(np.uint16) << np.uint16(t)
    return out


def pack_cells(cells, cat_ids, img_ids, A):
    """CocoBoxEval.cells()'s dict -- cells of any origin: the host loop, merged subsets, fallback cells -- as the flat arrays of
    include/ssd_hip.h: pack_order()'s dict plus 'matched', 'ignored' uint16 [A, nd] and 'gt_ignore' uint8 [A, ng].  Cells of
    categories or images outside cat_ids / img_ids are left out, as accumulate() leaves them out.  Every (category, image) must
    have its cell at all A area ranges with the same detections, which is what evaluate() produces."""
    cat_ids, img_ids = np.asarray(cat_ids, np.int64).reshape(-1), np.asarray(img_ids, np.int64).reshape(-1)
    keys, D, G = cells["keys"].reshape(-1, 3), np.asarray(cells["D"], np.int64), np.asarray(cells["G"], np.int64)
    d0, g0 = np.cumsum(D) - D, np.cumsum(G) - G
    keep = np.isin(keys[:, 0], cat_ids) & np.isin(keys[:, 2], img_ids)
    cat_at, img_at = np.searchsorted(cat_ids, keys[:, 0]), np.searchsorted(img_ids, keys[:, 2])
    out, first = None, None
    matched, ignored, gt_ignore = [], [], []
    for a in range(A):
        sel = np.nonzero(keep & (keys[:, 1] == a))[0]
        sel = sel[np.lexsort((img_at[sel], cat_at[sel]))]
        this = (cat_at[sel], img_at[sel], D[sel], G[sel])
        if a == 0:
            first = this
        elif not all(np.array_equal(x, y) for x, y in zip(this, first)):
            raise ValueError("area range %d holds other cells than area range 0: accumulate(device=) takes whole (category, image) cells" % a)
        rows, boxes = _ranges(d0[sel], D[sel]), _ranges(g0[sel], G[sel])
        if a == 0:
            out = _order(cat_at[sel], D[sel], G[sel], cells["scores"][rows], len(cat_ids))
        matched.append(words(cells["matched"][:, rows]))
        ignored.append(words(cells["ignored"][:, rows]))
        gt_ignore.append(cells["gt_ignore"][boxes].astype(np.uint8))
    out.update(matched=np.stack(matched), ignored=np.stack(ignored), gt_ignore=np.stack(gt_ignore))
    return out


def launch(segments_host, segments_dev, order, rank, matched, ignored, nd, gt_ignore, ng, T, A, max_dets, rec_thr, rec_thr_dev,
           precision, recall):
    """ssd_coco_accumulate on the current stream of the tensors' device.  segments_host: SEGMENT_DTYPE array; max_dets, rec_thr: host
    values; every other array a torch tensor on one GPU, of any dtype that holds the bytes: segments_dev [K * 32 bytes], order int32
    [nd], rank uint8 [nd], matched / ignored [A, nd] uint16 words, gt_ignore uint8 [A, ng], rec_thr_dev float64 [R], precision
    float64 [T, R, K, A, M], recall float64 [T, K, A, M]."""
    import torch
    from ._lib import check, lib
    from .metric_calls import stream
    segments_host = np.ascontiguousarray(segments_host, SEGMENT_DTYPE)
    max_dets = np.ascontiguousarray(max_dets, np.int32).reshape(-1)
    rec_thr = np.ascontiguousarray(rec_thr, np.float64).reshape(-1)
    dev = precision.device
    with torch.cuda.device(dev):
        check(lib().ssd_coco_accumulate(segments_host.ctypes.data, segments_dev.data_ptr(), len(segments_host), order.data_ptr(), rank.data_ptr(),
                                        matched.data_ptr(), ignored.data_ptr(), int(nd), gt_ignore.data_ptr(), int(ng), int(T), int(A),
                                        max_dets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(max_dets),
                                        rec_thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), rec_thr_dev.data_ptr(), len(rec_thr),
                                        precision.data_ptr(), recall.data_ptr(), stream(dev)))


def accumulate(q, matched, ignored, gt_ignore, T, A, max_dets, rec_thr, device, timings=None):
    """pack_order()'s dict q and the matching's outputs -- numpy arrays (uint16 [A, nd], uint8 [A, ng]: uploaded) or the tensors
    coco_match.match_device() left on `device` -- through the kernel -> precision float64 [T, R, K, A, M], recall float64 [T, K, A, M].
    timings: a dict that receives 'upload', 'launch' (HIP events) and 'download' in seconds."""
    import time
    import torch
    from . import metric_calls
    dev = metric_calls.device_of(device)
    up, tm = metric_calls.uploader(dev, "the matching's outputs", as_bytes=True), metric_calls.Timer(dev, timings is not None)
    K, M, R = len(q["segments"]), len(max_dets), len(rec_thr)
    rec_thr = np.ascontiguousarray(rec_thr, np.float64).reshape(-1)
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        segments_dev, order, rank, thr_dev = up(q["segments"]), up(q["order"]), up(q["rank"]), up(rec_thr)
        matched, ignored, gt_ignore = up(matched), up(ignored), up(gt_ignore)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        t1, e0 = tm.uploaded(), tm.mark()
        launch(q["segments"], segments_dev, order, rank, matched, ignored, q["nd"], gt_ignore, q["ng"], T, A, max_dets, rec_thr, thr_dev,
               precision, recall)
        launch_s = tm.seconds(e0, tm.mark())
        t2 = time.perf_counter()
        out = precision.cpu().numpy(), recall.cpu().numpy()
        if timings is not None:
            timings.update(upload=t1 - t0, launch=launch_s, download=time.perf_counter() - t2)
    return out
