"""The two kernels of the VOC-style metric restated in numpy, lane by lane (include/ssd_hip.h, "the VOC-style metric"; csrc/voc_match.hip):
match() scans cell by cell with the wave's choice of the first maximum -- lane l over the boxes l + 64 * j, the maximum of the lane
maxima, the smallest box among the lanes that hold it; curve() counts, scores and adds in the kernel's order -- 64 rows at a time,
the two sums as one chain of additions in ascending lane order with +0.0 from the lanes past the end.  evaluate_packed() stands in
for voc_match.evaluate_packed."""
import numpy as np


def _iou_row(d, g):
    """one detection [4] against boxes [G,4], (ymin, xmin, ymax, xmax): the header's operations, one at a time"""
    w = np.minimum(d[3], g[:, 3]) - np.maximum(d[1], g[:, 1])
    h = np.minimum(d[2], g[:, 2]) - np.maximum(d[0], g[:, 0])
    inter = np.where((w > 0) & (h > 0), w * h, 0.0)
    a_d = (d[3] - d[1]) * (d[2] - d[0])
    a_g = (g[:, 3] - g[:, 1]) * (g[:, 2] - g[:, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = inter / ((a_d + a_g) - inter)
    return np.where(inter > 0, q, 0.0)


def match(cells, det_box, det_pos, gt_box, thr, tp, tp_iou):
    """ssd_voc_match: writes tp[det_pos[i]] and tp_iou[det_pos[i]] of every packed detection in place, nothing else"""
    for cell in cells:
        d0, g0, D, G = int(cell["det_begin"]), int(cell["gt_begin"]), int(cell["D"]), int(cell["G"])
        g = gt_box[g0:g0 + G]
        taken = np.zeros((64, 64), bool)                               # [lane, j]
        for d in range(d0, d0 + D):
            top, first = -1.0, None
            if G:
                iou = _iou_row(det_box[d], g)
                lane_best = [(float(iou[l::64].max()), l + 64 * int(np.argmax(iou[l::64]))) for l in range(min(64, G))]
                top = max(v for v, _ in lane_best)
                first = min(k for v, k in lane_best if v == top)
            hit = top > 0.0 and top >= thr and not taken[first & 63, first >> 6]
            if hit:
                taken[first & 63, first >> 6] = True
            tp[det_pos[d]] = 1 if hit else 0
            tp_iou[det_pos[d]] = top if hit else 0.0


def curve(segments, tp, tp_iou, conf, result_dtype):
    """ssd_voc_curve -> result_dtype [len(segments)]"""
    out = np.zeros(len(segments), result_dtype)
    for l, seg in enumerate(segments):
        begin, n, num_gt = int(seg["begin"]), int(seg["count"]), float(int(seg["num_gt"]))
        carry, ap, iou_sum = 0, 0.0, 0.0
        lane_top = [(-np.inf, None, 0.0, 0.0)] * 64                   # (score, k, P, R): the lane's first maximum
        for k0 in range(0, n, 64):
            for lane in range(64):                                     # ascending lane order is the order of the additions
                k = k0 + lane
                t = k < n and tp[begin + k] != 0
                carry += bool(t)
                if k < n:
                    P, R = float(carry) / float(k + 1), float(carry) / num_gt
                    score = (P * R) * (1.0 - abs(P - R))
                    if score > lane_top[lane][0]:
                        lane_top[lane] = (score, k, P, R)
                ap = ap + (P * (R - float(carry - 1) / num_gt) if t else 0.0)
                iou_sum = iou_sum + (float(tp_iou[begin + k]) if t else 0.0)
        if n:
            best = max(v[0] for v in lane_top)
            _s, k, P, R = min((v for v in lane_top if v[0] == best), key=lambda v: v[1])
            out[l] = (ap, P, R, conf[begin + k], iou_sum / float(max(carry, 1)), carry, k, 0)
    return out


def evaluate_packed(p, thr, device=None, want_rows=False, timings=None):
    """voc_match.evaluate_packed with the restatement in the kernels' place (the oversize cells by voc_match.scan_cell, as there)"""
    from ssd_amd import voc_match
    tp, tp_iou = np.zeros(p["n_rows"], np.uint8), np.zeros(p["n_rows"], np.float64)
    for rows, dbox, gbox in p["fallback"]:
        tp[rows], tp_iou[rows] = voc_match.scan_cell(dbox, gbox, thr)
    match(p["cells"], p["det_box"], p["det_pos"], p["gt_box"], thr, tp, tp_iou)
    out = curve(p["segments"], tp, tp_iou, p["conf"], voc_match.RESULT_DTYPE)
    return (out, tp, tp_iou) if want_rows else out
