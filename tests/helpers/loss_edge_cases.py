"""Hand-built and seeded inputs for the matching kernels of loss.hip on an integer grid (corners in [0, 32], the domain of
tests/helpers/match_exact.py): arg-max ties by position, forced-match collisions, gt that overlap nothing, IoUs on the
thresholds, edge sizes, and a random fuzz on a small grid where thousands of IoUs are equal.  The host test and the GPU
test run the same generators.  A case is a dict: name, anchors [N,4] f32, boxes [B,G,4] f32, labels [B,G] i32, num [B]
i32, settings [(pos, neg)], levels (anchors per level, () for none).  Test infrastructure only."""
import numpy as np

BOTH = [(0.5, 0.5), (0.5, 0.25)]


def _case(name, anchors, boxes, labels, num, settings=BOTH, levels=()):
    anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 4)
    boxes = np.ascontiguousarray(boxes, np.float32)
    return {"name": name, "anchors": anchors, "boxes": boxes, "labels": np.ascontiguousarray(labels, np.int32),
            "num": np.asarray(num, np.int32), "settings": list(settings), "levels": tuple(int(v) for v in levels)}


def _labels(B, G, seed):
    return np.random.default_rng(seed).integers(0, 80, (B, G)).astype(np.int32)


def _rand_boxes(rng, n, lo, hi):
    """n boxes with integer corners in [lo, hi], ymin <= ymax and xmin <= xmax (zero areas included)."""
    y = np.sort(rng.integers(lo, hi + 1, (n, 2)), axis=1)
    x = np.sort(rng.integers(lo, hi + 1, (n, 2)), axis=1)
    return np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], axis=1).astype(np.float32)


def _cell(k, size):
    """Origin (y, x) of cell k of the 32 x 32 grid cut into cells of `size`."""
    per = 32 // size
    return (k // per) * size, (k % per) * size


def _filler(rng, n, positive=False):
    """Boxes inside the last row of 8 x 8 cells (y in [24, 32]): they never touch the cells the cases use."""
    if positive:
        y0, x0 = rng.integers(24, 32, n), rng.integers(0, 32, n)
        y = np.stack([y0, rng.integers(y0 + 1, 33)], axis=1)
        x = np.stack([x0, rng.integers(x0 + 1, 33)], axis=1)
    else:
        y = np.sort(rng.integers(24, 33, (n, 2)), axis=1)
        x = np.sort(rng.integers(0, 33, (n, 2)), axis=1)
    return np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], axis=1).astype(np.float32)


# ----------------------------------------------------------------------------- ties by position
ANCHOR_PAIRS = [(5, 6), (40, 104), (300, 556), (1100, 2123), (700, 1724), (2200, 6296), (0, 8199)]
GT_ROWS = (0, 255, 256, 511)


def anchor_ties():
    """One anchor box duplicated at (i, i+1), (i, i+64), (i, i+256), (i, i+1023), (i, i+1024), (i, i+4096), (0, N-1): the
    same thread's 4 anchors, another lane, another wave, another block of loss_best_anchor.  Each pair owns a 4 x 4 cell;
    a gt equal to the box (IoU 1) and a gt of IoU 1/3 with it sit at rows 0, 255, 256, 511 of some image.  At 1/3 only the
    forced anchor -- the lower index -- is matched; the other one is negative or ignored."""
    rng = np.random.default_rng(101)
    N, G, B = 8200, 512, 4
    anchors = _filler(rng, N)
    combos = []
    for k, (i, j) in enumerate(ANCHOR_PAIRS):
        oy, ox = _cell(k, 4)
        anchors[i] = anchors[j] = (oy, ox, oy + 2, ox + 2)
        combos.append((oy, ox, oy + 2, ox + 2))
    for k in range(len(ANCHOR_PAIRS)):
        oy, ox = _cell(k, 4)
        combos.append((oy, ox, oy + 4, ox + 3))                 # inter 4, union 12
    boxes = np.stack([_filler(rng, G, positive=True) for _ in range(B)])       # no empty gt: none picks anchor 0
    for c, box in enumerate(combos):
        boxes[c // 4, GT_ROWS[c % 4]] = box
    return [_case("anchor_ties", anchors, boxes, _labels(B, G, 1), [G] * B)]


GT_PAIRS = [(2, 3), (5, 9), (10, 266), (11, 268), (0, 599)]


def gt_ties():
    """Identical gt rows at (g, g+1) (two lanes of loss_anchor), (g, g+4) (one lane), (g, g+256) and (g, g+257) (the next
    gt tile, same or other lane) and (0, G-1), each pair in its own cell with an anchor equal to it (IoU 1) and one of
    IoU 1/3 (forced by neither: the equal anchor is their pick).  The lower row wins; the labels of the two rows differ."""
    rng = np.random.default_rng(102)
    N, G = 150, 600
    anchors = _filler(rng, N)
    boxes = _filler(rng, G)[None].copy()
    labels = _labels(1, G, 2)
    for k, (g, h) in enumerate(GT_PAIRS):
        oy, ox = _cell(k, 4)
        boxes[0, g] = boxes[0, h] = (oy, ox, oy + 2, ox + 2)
        labels[0, g], labels[0, h] = 2 * k, 2 * k + 1
        anchors[17 * k + 3] = (oy, ox, oy + 2, ox + 2)
        anchors[17 * k + 70] = (oy, ox, oy + 4, ox + 3)
    return [_case("gt_ties", anchors, boxes, labels, [G])]


# ----------------------------------------------------------------------------- forced-match collisions
FAIL = [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3)]                  # (h, w) of area <= 6: IoU <= 6/64 < 0.1 with the 8 x 8 anchor
PASS = [(7, 1), (4, 2), (3, 3), (5, 2), (4, 3)]                  # area >= 7: IoU >= 7/64 > 0.1
COLLISION_ROWS = {2: (0, 257), 3: (0, 5, 514), 5: (0, 1, 2, 259, 515)}


def collisions():
    """Two, three and five gt pick one 8 x 8 anchor A (they lie inside it and touch nothing else), at rows in different
    lanes and gt tiles.  The smallest row passes 0.1, or is the only one that fails it (A is still matched to it), or all
    fail (nothing is forced).  A has a plain match (IoU 40/64) to another gt X, whose own pick is an anchor equal to X:
    the forced match overrides it, and with all failing it stays."""
    rng = np.random.default_rng(103)
    N, G = 400, 600
    anchors = _filler(rng, N)
    boxes = _filler(rng, G)[None].copy()
    v = 0
    for k in (2, 3, 5):
        for kind in ("first_passes", "first_fails", "all_fail"):
            oy, ox = _cell(v, 8)
            anchors[13 * v + 1] = (oy, ox, oy + 8, ox + 8)                         # A
            anchors[13 * v + 200] = (oy, ox, oy + 8, ox + 5)                       # equal to X
            base = 20 + 7 * v
            boxes[0, 5 + v if v % 2 else 400 + v] = (oy, ox, oy + 8, ox + 5)                  # X: before the rows, or among them
            for n, r in enumerate(COLLISION_ROWS[k]):
                ok = {"first_passes": n != 1, "first_fails": n != 0, "all_fail": False}[kind]
                h, w = (PASS if ok else FAIL)[n]
                boxes[0, base + r] = (oy, ox + 5, oy + h, ox + 5 + w)              # inside A, beside X
            v += 1
    return [_case("collisions", anchors, boxes, _labels(1, G, 3), [G])]


# ----------------------------------------------------------------------------- a gt that overlaps nothing
def zero_overlap():
    """gt that overlap no anchor pick anchor 0 and are masked.  Anchor 0 is [0,0,8,8]; the cell [16,24] x [16,24] holds
    no anchor.  Image 0: such a gt alone.  1: at row 0 among ordinary gt, anchor 0 with a positive plain match.  2: at the
    last row, anchor 0 negative.  3: a passing gt at row 5 forces anchor 0 while a zero-IoU gt at row 2 picked it too:
    anchor 0 is matched to row 2.  4: zero-area gt (some equal to zero-area anchors, union 0) at rows 0, 1 and 6 among
    ordinary ones; row 2 equals anchor 0 and forces it: matched to row 0."""
    rng = np.random.default_rng(104)
    N, G, B = 90, 8, 5
    anchors = _filler(rng, N)
    anchors[0] = (0, 0, 8, 8)
    anchors[1] = (0, 8, 8, 16)
    anchors[2] = (8, 0, 12, 4)
    anchors[3] = (0, 0, 8, 6)                                   # the pick of image 1's gt 4: anchor 0 is forced by nobody there
    anchors[10] = (3, 20, 3, 27)                                # zero areas
    anchors[11] = (9, 9, 9, 9)
    anchors[12] = (3, 20, 3, 27)
    nothing = (17, 17, 22, 23)
    boxes = np.zeros((B, G, 4), np.float32)
    num = [1, G, G, G, G]
    boxes[0, 0] = nothing
    boxes[1] = _filler(rng, G)
    boxes[1, 0] = nothing
    boxes[1, 4] = (0, 0, 8, 6)                                  # IoU 3/4 with anchor 0
    boxes[2] = _filler(rng, G)
    boxes[2, 3] = (0, 8, 8, 16)
    boxes[2, G - 1] = nothing
    boxes[3] = _filler(rng, G)
    boxes[3, 2] = nothing
    boxes[3, 5] = (0, 0, 4, 8)                                  # IoU 1/2 with anchor 0, its pick
    boxes[4] = _filler(rng, G)
    boxes[4, 0] = (3, 20, 3, 27)
    boxes[4, 1] = (9, 9, 9, 9)
    boxes[4, 2] = (0, 0, 8, 8)
    boxes[4, 6] = (2, 2, 2, 6)                                  # zero area inside anchor 0
    boxes[4, 7] = (8, 0, 12, 4)
    return [_case("zero_overlap", anchors, boxes, _labels(B, G, 4), num)]


# ----------------------------------------------------------------------------- IoUs on the thresholds
PLAIN_STRIPS = [(16, 32), (15, 31), (8, 32), (7, 29), (16, 31), (8, 31)]     # probe width / gt width = the IoU
FORCED_STRIPS = [(3, 30), (2, 22), (3, 31), (3, 29), (1, 10), (1, 11)]


def thresholds():
    """Row y of the grid holds a probe anchor [y,0,y+1,a] and a gt [y,0,y+1,g]: IoU a/g exactly.  Plain strips have a
    second anchor equal to the gt (the gt's pick), so the probe keeps its plain value: 1/2 is matched, 15/31 is not; 1/4
    is ignored with neg = 0.25 and 7/29 negative.  Forced strips have the probe alone: 3/30 and 1/10 equal 0.1f and are
    forced, 2/22, 1/11 and 3/31 are not."""
    anchors, boxes = [], []
    for y, (a, g) in enumerate(PLAIN_STRIPS):
        anchors += [(y, 0, y + 1, a), (y, 0, y + 1, g)]
        boxes.append((y, 0, y + 1, g))
    for y, (a, g) in enumerate(FORCED_STRIPS, start=len(PLAIN_STRIPS)):
        anchors.append((y, 0, y + 1, a))
        boxes.append((y, 0, y + 1, g))
    G = len(boxes)
    return [_case("thresholds", anchors, np.array(boxes, np.float32)[None], _labels(1, G, 5), [G])]


# ----------------------------------------------------------------------------- sizes
SIZES_N = (1, 3, 63, 64, 65, 1023, 1024, 1025, 4097)
SIZES_G = (0, 1, 255, 256, 257, 4096)


def sizes(small=False):
    """N in SIZES_N against 40 gt; G in SIZES_G with gt_num full (G = 4096 against 3 000 anchors, 400 when `small`);
    gt_num of -3, 0, G and G + 5 in one batch, and of 7 and 13 of 20, with the rows beyond the count equal to anchors
    (they would win if they were read)."""
    out = []
    for N in SIZES_N:
        rng = np.random.default_rng(200 + N)
        out.append(_case("N=%d" % N, _rand_boxes(rng, N, 0, 12), _rand_boxes(rng, 2 * 40, 0, 12).reshape(2, 40, 4),
                         _labels(2, 40, N), [40, 17]))
    for G in SIZES_G:
        rng = np.random.default_rng(300 + G)
        N = (400 if small else 3000) if G == 4096 else 1500
        out.append(_case("G=%d" % G, _rand_boxes(rng, N, 0, 12), _rand_boxes(rng, 2 * G, 0, 12).reshape(2, G, 4),
                         _labels(2, G, G), [G, G]))
    rng = np.random.default_rng(400)
    anchors = _rand_boxes(rng, 700, 0, 12)
    anchors = anchors[(anchors[:, 2] > anchors[:, 0]) & (anchors[:, 3] > anchors[:, 1])]
    G = 20
    boxes = np.stack([anchors[b * G:(b + 1) * G] for b in range(4)])              # every row equals an anchor: IoU 1
    out.append(_case("gt_num clamped", anchors, boxes, _labels(4, G, 6), [-3, 0, G, G + 5]))
    boxes = _rand_boxes(rng, 2 * G, 0, 12).reshape(2, G, 4)
    boxes[0, 7:] = anchors[100:100 + G - 7]
    boxes[1, 13:] = anchors[200:200 + G - 13]
    out.append(_case("gt_num partial", anchors, boxes, _labels(2, G, 7), [7, 13]))
    return out


# ----------------------------------------------------------------------------- random grid fuzz
FUZZ_SEEDS = 24
FUZZ_SMALL = {0: (1, 5), 1: (7, 0), 2: (300, 1), 3: (6000, 2), 4: (1, 600), 5: (2, 19)}


def fuzz_case(seed):
    """N in [1, 6000] anchors, G in [0, 600] gt, integer corners in [0, 12]; B = 3 with different counts; n_levels in
    {0, 1, 5, 8} with random level sizes (zeros included) that sum to N.  Seeds in FUZZ_SMALL have N or G near 1."""
    rng = np.random.default_rng(1000 + seed)
    N, G = FUZZ_SMALL.get(seed, (int(rng.integers(500, 6001)), int(rng.integers(20, 601))))
    anchors = _rand_boxes(rng, N, 0, 12)
    boxes = _rand_boxes(rng, 3 * G, 0, 12).reshape(3, G, 4)
    num = [G, int(rng.integers(0, G + 1)), int(rng.integers(0, G + 1))]
    n_levels = (0, 1, 5, 8)[seed % 4]
    if n_levels <= 1:
        levels = [N] * n_levels
    else:
        cuts = np.sort(rng.integers(0, N + 1, n_levels - 1))
        cuts[rng.integers(0, n_levels - 1)] = cuts[0]                              # at least one empty level
        cuts = np.sort(cuts)
        levels = np.diff(np.concatenate([[0], cuts, [N]])).tolist()
    return _case("fuzz seed %d" % seed, anchors, boxes, _labels(3, G, seed), num, BOTH, levels)


def hand_built(small=False):
    return anchor_ties() + gt_ties() + collisions() + zero_overlap() + thresholds() + sizes(small)


# ----------------------------------------------------------------------------- loss values on generated anchors
PLANTED = [0.0, 1e-30, -1e-30, 16.6, -16.6, 17.4, -17.4, 88.0, -88.0, 104.0, -104.0, 720.0, -720.0, 1e4, -1e4]
MODERATE = PLANTED[:7]
DELTAS = [1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 0.0]
EQUAL_GT = 4                 # leading gt rows equal to an anchor: every regression target of that anchor is exactly 0


def value_inputs(anchors, C, counts, seed):
    """Random logits [B,N,C] and codes [B,N,4], gt jittered around random anchors (the first EQUAL_GT rows of an image
    with room for them equal to distinct anchors), labels in [0, C)."""
    rng = np.random.default_rng(seed)
    B, N, G = len(counts), len(anchors), max(max(counts), 1)
    logits = rng.normal(-3.0, 2.0, (B, N, C)).astype(np.float32)
    codes = rng.normal(0.0, 1.5, (B, N, 4)).astype(np.float32)
    boxes = np.zeros((B, G, 4), np.float32)
    labels = rng.integers(0, C, (B, G)).astype(np.int32)
    for b, n in enumerate(counts):
        idx = rng.choice(N, n, replace=False)
        a = anchors[idx].astype(np.float64)
        h, w = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cy = (a[:, 0] + a[:, 2]) / 2 + rng.normal(0, 0.15, n) * h
        cx = (a[:, 1] + a[:, 3]) / 2 + rng.normal(0, 0.15, n) * w
        h, w = h * np.exp(rng.normal(0, 0.3, n)), w * np.exp(rng.normal(0, 0.3, n))
        boxes[b, :n] = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(np.float32)
        if n >= EQUAL_GT:
            boxes[b, :EQUAL_GT] = anchors[idx[:EQUAL_GT]]
    return logits, codes, boxes, labels, np.array(counts, np.int32)


def plant_logits(logits, cls_targets, matches, values):
    """Writes every value, per image, on the target class of a matched anchor, on another class of a matched anchor (C > 1)
    and on a class of a background anchor; returns how many were planted."""
    B, N, C = logits.shape
    planted = 0
    for b in range(B):
        pos = np.flatnonzero(matches[b] >= 0)
        bg = np.flatnonzero(matches[b] == -1)
        for k, v in enumerate(values):
            if len(pos):
                a = pos[k % len(pos)]
                logits[b, a, cls_targets[b][a] - 1] = v
                planted += 1
                if C > 1:
                    a = pos[(k + 1) % len(pos)]
                    tc = cls_targets[b][a] - 1
                    logits[b, a, (tc + 1 + k % (C - 1)) % C] = v                # an offset in [1, C-1]: never the target
                    planted += 1
            logits[b, bg[7 * k], k % C] = v
            planted += 1
    return planted


def plant_codes(codes, reg_targets, matches):
    """On matched anchors whose four targets are exactly 0 (gt equal to the anchor), codes = DELTAS in turn, so that
    code - target is the delta itself; returns the [B,N] mask of those anchors."""
    mask = (matches >= 0) & (reg_targets == 0).all(axis=2)
    k = 0
    for b, a in np.argwhere(mask):
        for c in range(4):
            codes[b, a, c] = np.float32(DELTAS[k % len(DELTAS)])
            k += 1
    return mask
