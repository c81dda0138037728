"""An exact reference for match_boxes + create_targets' integer outputs (training_target_creation.py:48-176) on
INTEGER-coordinate boxes: anchors and gt with integer corners in [0, 32].  Intersection, areas and union are exact int64
and the IoU is np.float32(inter) / np.float32(uni), one correctly rounded division: for uni >= 1, uni + 1e-8f == uni in
fp32, so this is the value the kernel must compute, bit for bit (uni == 0, both boxes empty, gives 0).  Arg-max takes the
first index; the forced rule follows training_target_creation.py:105-126.  Shares no code with loss_ref.iou.

The matrix is built in chunks of anchors (G = 4096 against a few thousand anchors stays small).  Two conditions are
asserted on every chunk: the inputs are what the argument above needs (integers in range, so no pair has 0 < uni < 1),
and the order and the ties of the float32 IoUs are those of the exact ratios, compared by int64 cross-multiplication
(with uni <= 2048 two different ratios are at least 2^-22 apart, more than an fp32 ulp below 1).  Test infrastructure only."""
import numpy as np

f32 = np.float32
COORD_MAX = 32
SMALL_IOU = f32(0.1)


def _int_boxes(boxes, what):
    b = np.asarray(boxes)
    b = b.reshape(-1, 4)
    i = np.rint(b).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), b.astype(np.float64)), "%s: non-integer coordinates" % what
    assert i.size == 0 or (i.min() >= 0 and i.max() <= COORD_MAX), "%s: coordinates outside [0, %d]" % (what, COORD_MAX)
    assert (i[:, 2] >= i[:, 0]).all() and (i[:, 3] >= i[:, 1]).all(), "%s: ymax < ymin or xmax < xmin" % what
    return i


def inter_union(gt, anchors):
    """Exact int64 (inter, uni) [G, n] of integer boxes."""
    ih = np.maximum(0, np.minimum(gt[:, None, 2], anchors[None, :, 2]) - np.maximum(gt[:, None, 0], anchors[None, :, 0]))
    iw = np.maximum(0, np.minimum(gt[:, None, 3], anchors[None, :, 3]) - np.maximum(gt[:, None, 1], anchors[None, :, 1]))
    inter = ih * iw
    ag = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    aa = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    return inter, ag[:, None] + aa[None, :] - inter


def _similarity(inter, uni):
    """float32 IoU of a chunk, after the two assertions of the module docstring."""
    assert (inter >= 0).all() and (inter <= uni).all()
    assert not ((uni > 0) & (uni < 1)).any()                       # integers: stated, and checked, for the record
    safe = np.maximum(uni, 1)
    sim = (inter.astype(f32) / safe.astype(f32)).astype(f32)       # uni == 0 -> inter == 0 -> 0
    # the distinct (inter, uni) pairs, ordered; neighbours compared exactly and in float32
    key = np.unique(inter.ravel() * (4 * COORD_MAX * COORD_MAX) + safe.ravel())
    ki, ku = key // (4 * COORD_MAX * COORD_MAX), key % (4 * COORD_MAX * COORD_MAX)
    order = np.lexsort((ku, ki.astype(np.float64) / ku))
    ki, ku = ki[order], ku[order]
    kf = ki.astype(f32) / ku.astype(f32)
    lhs, rhs = ki[:-1] * ku[1:], ki[1:] * ku[:-1]                  # ratio[k] ? ratio[k+1]
    assert (lhs <= rhs).all(), "the float64 pre-order disagrees with the exact order"
    assert np.array_equal(lhs == rhs, kf[:-1] == kf[1:]) and np.array_equal(lhs < rhs, kf[:-1] < kf[1:]), \
        "float32 IoUs do not order like the exact ratios"
    return sim


def training_targets_multi(anchors, gt, labels, settings, chunk=2048, stats=None):
    """One image, several (pos, neg) threshold settings on one similarity matrix -> [(cls_targets, matches)] (int32 [N]).
    `stats`, a dict, receives the counts of anchors whose arg-max over the gt is tied at a positive IoU ('anchor_ties'),
    of gt whose arg-max over the anchors is tied at a positive IoU ('gt_ties'), and of anchors picked by two or more
    gt ('collisions')."""
    a = _int_boxes(anchors, "anchors")
    g = _int_boxes(gt, "gt")
    N, G = len(a), len(g)
    labels = np.asarray(labels, np.int64).reshape(-1)[:G]
    plain = [np.full((N,), -1, np.int64) for _ in settings]
    forced = np.zeros((N,), bool)
    row_id = np.full((N,), G, np.int64)
    if stats is not None:
        stats.update(anchor_ties=0, gt_ties=0, collisions=0)
    if G > 0:
        best_v = np.full((G,), -1.0, f32)                         # per gt: the largest IoU so far, its first anchor
        best_a = np.zeros((G,), np.int64)
        best_n = np.zeros((G,), np.int64)                         # how many anchors share it
        anchor_ties = 0
        for a0 in range(0, N, chunk):
            sim = _similarity(*inter_union(g, a[a0:a0 + chunk]))
            # per anchor (training_target_creation.py:88-100): the first gt of maximal IoU
            col = sim.max(axis=0)
            first = np.argmax(sim, axis=0)
            for m, (pos, neg) in zip(plain, settings):
                v = np.where(col >= f32(pos), first, -1)
                if f32(pos) != f32(neg):
                    v = np.where((col < f32(pos)) & ~(f32(neg) > col), -2, v)
                m[a0:a0 + chunk] = v
            anchor_ties += int((((sim == col[None, :]).sum(axis=0) > 1) & (col > 0)).sum())
            # per gt (:112): the first anchor of maximal IoU, chunks in ascending order
            row = sim.max(axis=1)
            arg = np.argmax(sim, axis=1) + a0
            cnt = (sim == row[:, None]).sum(axis=1)
            up = row > best_v
            same = row == best_v
            best_n = np.where(up, cnt, np.where(same, best_n + cnt, best_n))
            best_a = np.where(up, arg, best_a)
            best_v = np.where(up, row, best_v)
        # the forced overlay (:116-126): the row id from the unmasked one-hot, the mask from the gt that pass 0.1
        np.minimum.at(row_id, best_a, np.arange(G))
        forced[best_a[best_v >= SMALL_IOU]] = True
        if stats is not None:
            stats.update(anchor_ties=anchor_ties, gt_ties=int(((best_n > 1) & (best_v > 0)).sum()),
                         collisions=int((np.bincount(best_a, minlength=N) > 1).sum()))
    out = []
    for m in plain:
        matches = np.where(forced, row_id, m)
        cls = np.zeros((N,), np.int64)
        hit = matches >= 0
        cls[hit] = labels[matches[hit]] + 1
        out.append((cls.astype(np.int32), matches.astype(np.int32)))
    return out


def training_targets(anchors, gt, labels, pos=0.5, neg=0.5, chunk=2048, stats=None):
    """One image -> (cls_targets [N] int32, matches [N] int32)."""
    return training_targets_multi(anchors, gt, labels, [(pos, neg)], chunk, stats)[0]
