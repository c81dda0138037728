"""The reference of tiled detection (include/ssd_hip.h, block "tiled detection") in numpy: the grid restated from its formulas, the
fp32 move of a tile's boxes to frame coordinates, and the merge -- per (frame, class) the candidates in source order through the
oracle's NMS (oracle.ops.nms: orc_nms).  merge_brute restates the selection a second time without the oracle: a Python sort, an
O(n^2) loop and the IoU comparison in numpy float32 scalars; it also reports which kept box suppressed which candidate."""
import math

import numpy as np

F32 = np.float32


def grid(H, W, th, tw, overlap):
    """-> (ys, xs): top rows and left columns of the tiles"""
    oy, ox = int(overlap * th), int(overlap * tw)
    sy, sx = th - oy, tw - ox
    assert sy >= 1 and sx >= 1 and H >= th and W >= tw
    ny, nx = 1 + math.ceil((H - th) / sy), 1 + math.ceil((W - tw) / sx)
    return [min(i * sy, H - th) for i in range(ny)], [min(i * sx, W - tw) for i in range(nx)]


def crops(frames, th, tw, overlap):
    """frames uint8 [F,H,W,3] -> [F * ny * nx, th, tw, 3] by numpy slicing, in tile order"""
    ys, xs = grid(frames.shape[1], frames.shape[2], th, tw, overlap)
    return np.stack([fr[y:y + th, x:x + tw] for fr in frames for y in ys for x in xs])


def split(rec):
    """views of a record block [B, 6T+1] int32: boxes [B,T,4] f32, labels [B,T], scores [B,T] f32, num [B]"""
    B, words = rec.shape
    T = (words - 1) // 6
    return rec[:, :4 * T].view(F32).reshape(B, T, 4), rec[:, 5 * T:6 * T], rec[:, 4 * T:5 * T].view(F32), rec[:, 6 * T]


def records(rows_per_source, T):
    """rows_per_source: a list (one entry per record) of lists of (label, score, (ymin, xmin, ymax, xmax)) -> [B, 6T+1] int32"""
    rec = np.zeros((len(rows_per_source), 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(rec)
    for s, rows in enumerate(rows_per_source):
        num[s] = len(rows)
        for r, (lb, sc, box) in enumerate(rows):
            boxes[s, r], labels[s, r], scores[s, r] = np.asarray(box, F32), lb, F32(sc)
    return rec


def to_frame(boxes, y0, x0, th, tw, H, W):
    """tile-normalised boxes [n,4] -> frame-normalised, one fp32 operation at a time"""
    out = np.empty_like(boxes)
    for k, (side, o, full) in enumerate(((th, y0, H), (tw, x0, W), (th, y0, H), (tw, x0, W))):
        out[:, k] = ((boxes[:, k] * F32(side)) + F32(o)) / F32(full)
    return out


def candidates(tile_rec, full_rec, f, c, H, W, th, tw, overlap):
    """-> (boxes [n,4] in frame coordinates, scores [n], source [n]) of (frame f, class c) in candidate order"""
    ys, xs = grid(H, W, th, tw, overlap)
    nt = len(ys) * len(xs)
    T = (tile_rec.shape[1] - 1) // 6
    bs, ss, src = [], [], []
    sources = [(tile_rec[f * nt + s:f * nt + s + 1], s) for s in range(nt)] + ([(full_rec[f:f + 1], nt)] if full_rec is not None else [])
    for rec, s in sources:
        boxes, labels, scores, num = split(rec)
        n = min(max(int(num[0]), 0), T)
        pick = np.nonzero(labels[0, :n] == c)[0]
        b = boxes[0, pick]
        if s < nt:
            b = to_frame(b, ys[s // len(xs)], xs[s % len(xs)], th, tw, H, W)
        bs.append(b)
        ss.append(scores[0, pick])
        src.append(np.full(len(pick), s, np.int64))
    return np.concatenate(bs).reshape(-1, 4).astype(F32), np.concatenate(ss).astype(F32), np.concatenate(src)


def iou_greater(bi, bj, thr):
    """IOUGreaterThanThreshold in numpy float32 scalars, operation for operation"""
    ymin_i, xmin_i, ymax_i, xmax_i = min(bi[0], bi[2]), min(bi[1], bi[3]), max(bi[0], bi[2]), max(bi[1], bi[3])
    ymin_j, xmin_j, ymax_j, xmax_j = min(bj[0], bj[2]), min(bj[1], bj[3]), max(bj[0], bj[2]), max(bj[1], bj[3])
    area_i = F32(ymax_i - ymin_i) * F32(xmax_i - xmin_i)
    area_j = F32(ymax_j - ymin_j) * F32(xmax_j - xmin_j)
    if area_i <= 0 or area_j <= 0:
        return False
    ih = max(F32(min(ymax_i, ymax_j) - max(ymin_i, ymin_j)), F32(0))
    iw = max(F32(min(xmax_i, xmax_j) - max(xmin_i, xmin_j)), F32(0))
    inter = F32(ih * iw)
    uni = F32(F32(area_i + area_j) - inter)
    return bool(F32(inter / uni) > F32(thr))


def select_brute(boxes, scores, m, thr):
    """-> (selected candidate indices, [(suppressed candidate, the kept candidate that suppressed it)])"""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    kept, dropped = [], []
    for i in order:
        if len(kept) == m:
            break
        by = next((j for j in reversed(kept) if iou_greater(boxes[i], boxes[j], thr)), None)
        if by is None:
            kept.append(i)
        else:
            dropped.append((i, by))
    return kept, dropped


def _merge(select, tile_rec, full_rec, F, H, W, th, tw, overlap, C, m):
    T = C * m
    out = np.zeros((F, 6 * T + 1), np.int32)
    boxes, labels, scores, num = split(out)
    for f in range(F):
        k = 0
        for c in range(C):
            b, s, _src = candidates(tile_rec, full_rec, f, c, H, W, th, tw, overlap)
            for i in select(b, s):
                boxes[f, k], labels[f, k], scores[f, k] = b[i], c, s[i]
                k += 1
        num[f] = k
    return out


def merge(ops, tile_rec, full_rec, F, H, W, th, tw, overlap, C, m, thr):
    """the merged records [F, 6T+1]; ops: oracle.ops"""
    def select(b, s):
        return ops.nms(b, s, m, thr, -np.inf) if len(s) else []
    return _merge(select, tile_rec, full_rec, F, H, W, th, tw, overlap, C, m)


def merge_brute(tile_rec, full_rec, F, H, W, th, tw, overlap, C, m, thr):
    return _merge(lambda b, s: select_brute(b, s, m, thr)[0], tile_rec, full_rec, F, H, W, th, tw, overlap, C, m)


def cross_source_stats(tile_rec, full_rec, F, H, W, th, tw, overlap, C, m, thr):
    """-> (suppressions where the candidate and the box that suppressed it come from different TILES, the largest number of
    sources one (frame, class) draws its candidates from)"""
    nt = tile_rec.shape[0] // F
    cross = most = 0
    for f in range(F):
        for c in range(C):
            b, s, src = candidates(tile_rec, full_rec, f, c, H, W, th, tw, overlap)
            most = max(most, len(set(src.tolist())))
            for i, j in select_brute(b, s, m, thr)[1]:
                cross += src[i] != src[j] and src[i] < nt and src[j] < nt
    return int(cross), most
