"""A numpy restatement of the EVAL loss for the tests (training_target_creation.py:5-176, box_utils.py:14-113,
losses.py, ssd.py:71-133): every TF op one float32 op, exp / log / log1p / sigmoid / pow evaluated in float64 and
rounded once, first index on argmax ties (include/ssd_hip.h).  `losses_f64` evaluates the same formulas in float64
throughout (the yardstick of the scalars).  Test infrastructure only."""
import numpy as np

f32 = np.float32


def iou(gt, anchors):
    """box_utils.py:14-66 in float32: [G, N]."""
    gt = np.asarray(gt, f32).reshape(-1, 4)
    a = np.asarray(anchors, f32).reshape(-1, 4)
    ih = np.maximum(f32(0), np.minimum(gt[:, None, 2], a[None, :, 2]) - np.maximum(gt[:, None, 0], a[None, :, 0]))
    iw = np.maximum(f32(0), np.minimum(gt[:, None, 3], a[None, :, 3]) - np.maximum(gt[:, None, 1], a[None, :, 1]))
    inter = ih * iw
    ag = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    uni = (ag[:, None] + aa[None, :]) - inter
    return np.clip(inter / (uni + f32(1e-8)), f32(0), f32(1)).astype(f32)


def match_boxes(anchors, gt, pos=0.5, neg=0.5):
    """training_target_creation.py:48-130 (force_match_groundtruth=True) for G > 0."""
    sim = iou(gt, anchors)
    G, N = sim.shape
    matches = np.argmax(sim, axis=0).astype(np.int64)            # numpy: first index on ties
    vals = sim.max(axis=0)
    is_pos = vals >= f32(pos)
    if f32(pos) == f32(neg):
        matches = np.where(is_pos, matches, -1)
    else:
        is_neg = f32(neg) > vals
        matches = np.where(is_pos, matches, np.where(is_neg, -1, -2))
    forced = np.argmax(sim, axis=1)
    ok = sim.max(axis=1) >= f32(0.1)
    onehot = np.zeros((G, N), np.int64)
    onehot[np.arange(G), forced] = 1
    row_ids = np.argmax(onehot, axis=0)                          # the smallest gt that picked the anchor (unmasked)
    mask = (onehot * ok[:, None].astype(np.int64)).max(axis=0) > 0
    return np.where(mask, row_ids, matches).astype(np.int32)


def encode(boxes, anchors):
    """box_utils.py:80-113 in float32 (log correctly rounded)."""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    a = np.asarray(anchors, f32).reshape(-1, 4)
    ha, wa = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cya, cxa = a[:, 0] + f32(0.5) * ha, a[:, 1] + f32(0.5) * wa
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cy, cx = b[:, 0] + f32(0.5) * h, b[:, 1] + f32(0.5) * w
    eps = f32(1e-8)
    ha, wa, h, w = ha + eps, wa + eps, h + eps, w + eps
    ty = (cy - cya) / ha * f32(10.0)
    tx = (cx - cxa) / wa * f32(10.0)
    th = np.log((h / ha).astype(np.float64)).astype(f32) * f32(5.0)
    tw = np.log((w / wa).astype(np.float64)).astype(f32) * f32(5.0)
    return np.stack([ty, tx, th, tw], axis=1).astype(f32)


def training_targets(anchors, gt, labels, pos=0.5, neg=0.5):
    """get_training_targets of one image -> reg_targets [N,4], cls_targets [N], matches [N]."""
    N = len(anchors)
    gt = np.asarray(gt, f32).reshape(-1, 4)
    if len(gt) == 0:
        matches = np.full((N,), -1, np.int32)
    else:
        matches = match_boxes(anchors, gt, pos, neg)
    reg = np.zeros((N, 4), f32)
    cls = np.zeros((N,), np.int32)
    m = matches >= 0
    if m.any():
        reg[m] = encode(gt[matches[m]], np.asarray(anchors, f32)[m])
        cls[m] = np.asarray(labels, np.int32)[matches[m]] + 1
    return reg, cls, matches


def focal_terms(logits, cls_targets, gamma=2.0, alpha=0.25):
    """losses.py:22-49 element-wise in float32 ops: [N, C]."""
    x = np.asarray(logits, f32)
    C = x.shape[1]
    z = (np.asarray(cls_targets)[:, None] == np.arange(1, C + 1)[None, :])
    zf = z.astype(f32)
    relu = np.where(x >= 0, x, f32(0))
    e = np.exp(-np.abs(x).astype(np.float64)).astype(f32)
    nlpt = (relu - x * zf) + np.log1p(e.astype(np.float64)).astype(f32)
    p = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(f32)
    pt = np.where(z, p, f32(1) - p)
    mod = np.power((f32(1) - pt).astype(np.float64), float(f32(gamma))).astype(f32)
    w = np.where(z, f32(alpha) * nlpt, f32(1.0 - alpha) * nlpt)
    return (mod * w).astype(f32)


def smooth_l1(codes, targets):
    d = np.abs(np.asarray(codes, f32) - np.asarray(targets, f32))
    return np.where(d < f32(1), f32(0.5) * (d * d), d - f32(0.5)).astype(f32)


def image_losses(logits, codes, anchors, gt, labels, gamma=2.0, alpha=0.25, pos=0.5, neg=0.5):
    """One image -> (cls_losses [N], loc_losses [N], matches [N]) in float32 (class / code sums in float64, rounded once)."""
    reg, cls, matches = training_targets(anchors, gt, labels, pos, neg)
    cl = focal_terms(logits, cls, gamma, alpha).astype(np.float64).sum(axis=1).astype(f32)
    ll = smooth_l1(codes, reg).astype(np.float64).sum(axis=1).astype(f32)
    cl = (matches >= -1).astype(f32) * cl
    ll = (matches >= 0).astype(f32) * ll
    return cl, ll, matches


def batch_losses(logits, codes, anchors, boxes, labels, num, **kw):
    """ssd.py:71-133 over a batch -> (losses [2] float32, per_image [B,3] float64 sums, per-anchor cls [B,N], loc [B,N])."""
    B = len(logits)
    cls_l, loc_l, per = [], [], []
    for b in range(B):
        n = int(num[b])
        c, l, m = image_losses(logits[b], codes[b], anchors, boxes[b][:n], labels[b][:n], **kw)
        cls_l.append(c)
        loc_l.append(l)
        per.append((l.astype(np.float64).sum(), c.astype(np.float64).sum(), float((m >= 0).sum())))
    per = np.array(per, np.float64)
    norm = max(f32(per[:, 2].sum()), f32(1))
    losses = np.array([f32(per[:, 0].sum()) / norm, f32(per[:, 1].sum()) / norm], f32)
    return losses, per, np.stack(cls_l), np.stack(loc_l)


def losses_f64(logits, codes, anchors, boxes, labels, num, gamma=2.0, alpha=0.25, pos=0.5, neg=0.5):
    """The same losses with the targets of the float32 restatement and every loss op in float64: [2]."""
    B = len(logits)
    tot_l = tot_c = tot_m = 0.0
    for b in range(B):
        n = int(num[b])
        reg, cls, m = training_targets(anchors, boxes[b][:n], labels[b][:n], pos, neg)
        x = np.asarray(logits[b], np.float64)
        C = x.shape[1]
        z = (cls[:, None] == np.arange(1, C + 1)[None, :])
        nlpt = np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))
        p = 1.0 / (1.0 + np.exp(-x))
        pt = np.where(z, p, 1 - p)
        fl = np.power(1 - pt, gamma) * np.where(z, alpha, 1 - alpha) * nlpt
        tot_c += (fl.sum(axis=1) * (m >= -1)).sum()
        d = np.abs(np.asarray(codes[b], np.float64) - reg.astype(np.float64))
        sl = np.where(d < 1, 0.5 * d * d, d - 0.5)
        tot_l += (sl.sum(axis=1) * (m >= 0)).sum()
        tot_m += (m >= 0).sum()
    norm = max(tot_m, 1.0)
    return np.array([tot_l / norm, tot_c / norm])
