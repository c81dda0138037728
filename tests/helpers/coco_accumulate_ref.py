"""ssd_coco_accumulate restated in numpy float64 on the flat arrays, from include/ssd_hip.h, block "the COCO accumulation" (not from
CocoBoxEval.accumulate, which tests/test_coco_accumulate_host.py compares it with): per (k, a) npig; per (k, a, m, t) the
participating rows in global order, integer cumulative counts, rc and pr one IEEE operation at a time, the suffix maximum, and the
sampling at the first row with rc_j >= rec_thr[r] -- the block's own definition.  first_count() restates c_r, the form the kernel
samples by; the host test compares it with the definition."""
import numpy as np

EPS = np.float64(2.0) ** -52


def first_count(thr, npig):
    """c_r as the kernel forms it: the estimate ceil(thr * npig), corrected by the exact test double(c) / double(npig) >= thr on its
    neighbours -> the smallest integer c >= 0 that passes; 2^31, which no count reaches, when that is further than a count can go."""
    thr, dn, cap = np.float64(thr), np.float64(npig), 2 ** 31
    if not thr > 0.0:
        return 0
    c = int(min(np.ceil(thr * dn), np.float64(cap)))
    while c > 0 and np.float64(c - 1) / dn >= thr:
        c -= 1
    while c < cap and np.float64(c) / dn < thr:
        c += 1
    return c


def accumulate(segments, order, rank, matched, ignored, gt_ignore, T, max_dets, rec_thr):
    """segments: records with det_begin, det_count, gt_begin, gt_count [K]; order int32 [nd]; rank uint8 [nd]; matched / ignored
    uint16 [A, nd], bit t; gt_ignore uint8 [A, ng] -> precision float64 [T, R, K, A, M], recall float64 [T, K, A, M]"""
    rec_thr = np.asarray(rec_thr, np.float64)
    K, A, M, R = len(segments), matched.shape[0], len(max_dets), len(rec_thr)
    precision = np.full((T, R, K, A, M), -1.0)
    recall = np.full((T, K, A, M), -1.0)
    for k, seg in enumerate(segments):
        d0, dc, g0, gc = int(seg["det_begin"]), int(seg["det_count"]), int(seg["gt_begin"]), int(seg["gt_count"])
        rows_all = order[d0:d0 + dc].astype(np.int64)
        for a in range(A):
            npig = int(np.count_nonzero(gt_ignore[a, g0:g0 + gc] == 0))
            if npig == 0:
                continue
            for m, maxdet in enumerate(max_dets):
                rows = rows_all[rank[rows_all] < maxdet]
                n = len(rows)
                mw, iw = matched[a, rows].astype(np.int64), ignored[a, rows].astype(np.int64)
                for t in range(T):
                    mt, it = (mw >> t) & 1, (iw >> t) & 1
                    tp = np.cumsum(mt & (1 - it))                       # integers
                    fp = np.cumsum((1 - mt) & (1 - it))
                    if n == 0:
                        recall[t, k, a, m] = 0.0
                        precision[t, :, k, a, m] = 0.0
                        continue
                    tpd, fpd = tp.astype(np.float64), fp.astype(np.float64)
                    rc = tpd / np.float64(npig)
                    pr = tpd / ((fpd + tpd) + EPS)
                    E = np.maximum.accumulate(pr[::-1])[::-1]
                    recall[t, k, a, m] = rc[-1]
                    pos = np.searchsorted(rc, rec_thr, side="left")     # the first row with rc_j >= rec_thr[r]
                    ok = pos < n
                    q = np.zeros(R)
                    q[ok] = E[pos[ok]]
                    precision[t, :, k, a, m] = q
    return precision, recall
