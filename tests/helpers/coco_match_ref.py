"""The kernel's per-lane algorithm (csrc/coco_match.hip; semantics: include/ssd_hip.h, "the COCO box matching") restated in
numpy on the packed arrays: IoUs one float64 operation at a time, the scan order as two passes over the groundtruth boxes in
annotation order (not ignored, then ignored), `taken` as a bit mask, and the packed uint16 outputs with bit t per threshold."""
import numpy as np


def iou_xywh(d, g, crowd):
    """One pair, the header's operations in the header's order (numpy float64 scalars: every operation rounded once)."""
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if not (w > 0 and h > 0):
        return np.float64(0.0)
    inter = w * h
    da = dw * dh
    ga = gw * gh
    union = da if crowd else (da + ga) - inter
    return inter / union


def match(cells, det_box, det_area, gt_box, gt_area, gt_crowd, thr, area_rng, want_iou=False):
    """-> matched, ignored uint16 [A, nd] (bit t), gt_ignore uint8 [A, ng] in scan order (and the IoU dump, cell-major [D, G] in
    annotation order, with want_iou).  Rows of no cell keep 0xFFFF / 0xFF."""
    T, A = len(thr), len(area_rng)
    nd, ng = len(det_area), len(gt_area)
    matched = np.full((A, nd), 0xFFFF, np.uint16)
    ignored = np.full((A, nd), 0xFFFF, np.uint16)
    gt_ignore = np.full((A, ng), 0xFF, np.uint8)
    dump = []
    for cell in cells:
        d0, g0, D, G = int(cell["det_begin"]), int(cell["gt_begin"]), int(cell["D"]), int(cell["G"])
        crowd = [bool(c) for c in gt_crowd[g0:g0 + G]]
        iou = [[iou_xywh(det_box[d0 + d], gt_box[g0 + g], crowd[g]) for g in range(G)] for d in range(D)]
        dump += [v for row in iou for v in row]
        matched[:, d0:d0 + D] = 0
        ignored[:, d0:d0 + D] = 0
        for a, (lo, hi) in enumerate(area_rng):
            ig = [crowd[g] or gt_area[g0 + g] < lo or gt_area[g0 + g] > hi for g in range(G)]
            regular = G - sum(ig)
            gt_ignore[a, g0:g0 + G] = [j >= regular for j in range(G)]
            for t in range(T):                                  # lane a * T + t
                taken = 0
                for d in range(D):
                    best, m, m_ig, stop = thr[t], -1, False, False
                    for in_pass in (False, True):
                        for g in range(G):
                            if stop or ig[g] != in_pass or ((taken >> g) & 1 and not crowd[g]):
                                continue
                            if m >= 0 and not m_ig and ig[g]:
                                stop = True
                                continue
                            if not iou[d][g] < best:
                                best, m, m_ig = iou[d][g], g, ig[g]
                    hit = m >= 0
                    if hit:
                        taken |= 1 << m
                    ign = m_ig if hit else bool(det_area[d0 + d] < lo or det_area[d0 + d] > hi)
                    matched[a, d0 + d] |= np.uint16(int(hit) << t)
                    ignored[a, d0 + d] |= np.uint16(int(ign) << t)
    out = (matched, ignored, gt_ignore)
    return out + (np.array(dump, np.float64),) if want_iou else out
