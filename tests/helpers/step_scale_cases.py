"""The cases of tests/test_gpu_step_scale.py and their premises (tests/test_step_scale_host.py asserts them without a GPU): tables for
ssd_train_norms, ssd_train_histograms and the gradient exchange at the sizes where their second code paths begin -- stage 2's
64-partial chunks, a second and a third pass of the 2 048-block grid, elements and slices past 2^32 bytes, a table of many small rows
-- and the tiled expectations of the two cases too large to restate element by element.  Everything here is numpy on the three
restatements (helpers/train_norms_ref.py, histogram_ref.py, train_reduce_ref.py); the package is imported only for the names and counts
of case B1."""
import collections
import functools

import numpy as np

from helpers import histogram_ref as href
from helpers import train_norms_ref as nref
from helpers import train_reduce_ref as rref

f32, f64 = np.float32, np.float64
BLOCK = nref.BLOCK                       # SSD_UPDATE_BLOCK_ELEMS
GRID = 2048                              # TBL_MAX_GRID of csrc/train_table.h: hardware blocks of one pass
CHUNK = 64                               # TBL_WAVE: partials stage 2 loads per trip
WD = 0.5                                 # the histogram tests' weight_decay: g + 0.5 * w lands in other buckets than g
GIB = 2 ** 30
MOBILENET = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80}
SHUFFLENET = {"backbone": "shufflenet", "depth_multiplier": 1.0, "num_classes": 80}
BACKBONES = {"mobilenet": MOBILENET, "shufflenet": SHUFFLENET}

# one row of the update's table: host arrays (grad None: a NULL gradient), the float offsets of w and grad inside their 16-byte groups
Row = collections.namedtuple("Row", "w g wo go decay")


def values(rng, n):
    """The GPU suites' _values(): a normal times 2^U[-40, 40], so that a wrong order of the additions shows in the last bits."""
    return (rng.normal(0, 1, n) * np.exp2(rng.integers(-40, 41, n))).astype(f32)


def nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(f32)[0]


def norms_specs(rows):
    """test_gpu_train_norms._table's input."""
    return [(r.w, r.g, r.wo, r.go) for r in rows]


def hist_specs(rows):
    """test_gpu_train_histograms._table's input."""
    return [tuple(r) for r in rows]


# ----------------------------------------------------------------------------- the work list of a table
def row_blocks(rows):
    return [nref.n_blocks(len(r.w), r.wo) for r in rows]


def first_blocks(rows):
    blocks = np.array(row_blocks(rows), np.int64)
    return (np.cumsum(blocks) - blocks).tolist()


def passes(total_blocks):
    """Iterations of `for (c = blockIdx.x; c < total_blocks; c += gridDim.x)` that hardware block 0 runs."""
    return -(-total_blocks // min(max(total_blocks, 1), GRID))


def chunks(blocks):
    """Trips of stage 2's loop over one row's partials."""
    return -(-blocks // CHUNK)


def block_range(row, b):
    """The elements [lo, hi) of `row` that lie in its block b (blocks count from the 16-byte boundary at or below w)."""
    return max(0, b * BLOCK - row.wo), min(len(row.w), (b + 1) * BLOCK - row.wo)


def row_of_block(rows, c):
    """The kernels' search: the last row whose first_block <= c."""
    first = first_blocks(rows)
    return max(t for t in range(len(rows)) if first[t] <= c)


def buckets(x):
    """The distinct buckets the finite elements of x fall into."""
    x = np.asarray(x, f32)
    return np.unique(np.searchsorted(href.LIMITS, x[np.isfinite(x)].astype(f64), side="right"))


# ----------------------------------------------------------------------------- A. stage 2 at its chunk boundaries
A_BLOCKS = (63, 64, 65, 127, 128, 129, 256, 257)
A_ONE_ELEMENT = (65, 129, 257)           # count + pad = k * 4096 + 1: the chunk after a full one ends on a one-element block
A_EXTREME = (f32(2.0 ** 45), f32(2.0 ** 46))     # |min| = max of the w plane, of the gradient: above every drawn value and sum


def _plant_a(x, row, nb, big, single):
    """A NaN in the last block of the first chunk and in the first block of the second, the minimum in block 64, the maximum in the
    last block.  In the 65-block row block 64 is the last block and holds ONE element: it takes `single` of the two extremes, the
    other one goes to block 63 and the second NaN is left out."""
    lo, hi = block_range(row, min(CHUNK, nb) - 1)
    x[lo + 11] = np.nan
    last = block_range(row, nb - 1)
    if nb > CHUNK:
        lo, hi = block_range(row, CHUNK)
        if hi - lo == 1:
            x[lo] = -big if single == "min" else big
            lo, hi = block_range(row, CHUNK - 1)
            x[hi - 1] = big if single == "min" else -big
            return
        x[lo] = np.nan
        x[lo + 1] = -big
    x[last[1] - 1] = big


@functools.lru_cache(maxsize=None)
def case_a():
    """Eight rows of 63 .. 257 blocks at w offsets 0..3 in turn, every other one with a gradient (decay 1), and a 4096-element decaying
    row whose gradient plane overflows only through weight_decay * w: 1 090 blocks, one grid pass."""
    rng = np.random.default_rng(41)
    rows = []
    for t, nb in enumerate(A_BLOCKS):
        wo = t % 4
        if nb in A_ONE_ELEMENT:
            virtual = (nb - 1) * BLOCK + 1
        else:
            virtual = nb * BLOCK if nb % CHUNK == 0 else nb * BLOCK - 5 - t
        n = virtual - wo
        has_grad = t % 2 == 0
        row = Row(values(rng, n), values(rng, n) if has_grad else None, wo, wo if t % 4 == 0 else (wo + 1) % 4, int(has_grad))
        _plant_a(row.w, row, nb, A_EXTREME[0], "min")
        if has_grad:
            _plant_a(row.g, row, nb, A_EXTREME[1], "max")
        rows.append(row)
    w, g = values(rng, BLOCK), values(rng, BLOCK)
    w[[100, 4095]] = [3e38, -3e38]                                   # finite, and so is g: g + 0.5 * w is +inf and -inf
    g[[100, 4095]] = [3e38, -3e38]
    rows.append(Row(w, g, 0, 0, 1))
    return tuple(rows)


# ----------------------------------------------------------------------------- B1. the whole trainable set: two grid passes
@functools.lru_cache(maxsize=1)
def case_b1(backbone, views):
    """Every trainable tensor of the architecture (names and counts of train_step.trainable_names and ssd.synthetic_weights), about
    one in ten without a gradient, decay by train_step.decays; `views`: tensor i starts 1 + i % 3 floats past a 16-byte boundary.
    Every fifth gradient is of another alignment class than its w.  -> (names, rows)"""
    import ssd_amd
    from ssd_amd import train_step
    params = BACKBONES[backbone]
    W = ssd_amd.synthetic_weights(params, seed=11)
    names = train_step.trainable_names(params)
    rng = np.random.default_rng(51 + len(backbone) + int(views))
    rows = []
    for i, name in enumerate(names):
        n = int(W[name].size)
        wo = 1 + i % 3 if views else 0
        g = None if rng.random() < 0.1 else values(rng, n)
        rows.append(Row(values(rng, n), g, wo, (wo + 1) % 4 if i % 5 == 4 else wo, int(train_step.decays(name))))
    return tuple(names), tuple(rows)


# ----------------------------------------------------------------------------- B2. 2 * 2048 + 300 blocks: three grid passes
B2_THIRD = 300                                                       # hardware blocks 0 .. 299 make a third trip
B2_TOTAL = 2 * GRID + B2_THIRD
# (kind, blocks, w offset, gradient: None / "same" / "other" alignment class, decay, floats the last block falls short of 4096)
B2_LAYOUT = (
    ("wide", 129, 1, "same", 1, 7),          # [0, 129)
    ("wide", 171, 0, "other", 0, 0),         # [129, 300)
    ("wide", 1000, 2, None, 0, 4095),        # [300, 1300): ends on a one-element block
    ("wide", 740, 3, "same", 0, 100),        # [1300, 2040)
    ("const", 110, 0, "same", 0, 33),        # [2040, 2150): straddles work blocks 2047 and 2048
    ("empty", 0, 0, "same", 1, 0),           # first_block 2150
    ("const", 1, 3, "same", 0, 4092),        # [2150, 2151): one element
    ("const", 197, 2, "other", 1, 1),        # [2151, 2348)
    ("wide", 900, 1, "same", 1, 2000),       # [2348, 3248)
    ("wide", 842, 0, None, 0, 0),            # [3248, 4090)
    ("wide", 100, 2, "same", 1, 9),          # [4090, 4190): straddles work blocks 4095 and 4096
    ("wide", 206, 3, "other", 0, 4000),      # [4190, 4396)
)
B2_CONSTANTS = {4: (0.125, -3.0), 6: (7.5, -2e-5), 7: (-1e-3, 2.0)}  # (w, grad) of the constant rows: other buckets in either plane


@functools.lru_cache(maxsize=None)
def case_b2():
    rng = np.random.default_rng(61)
    rows = []
    for t, (kind, nb, wo, grad, decay, short) in enumerate(B2_LAYOUT):
        n = 0 if kind == "empty" else nb * BLOCK - short - wo
        if kind == "const":
            w, g = np.full(n, B2_CONSTANTS[t][0], f32), np.full(n, B2_CONSTANTS[t][1], f32)
        else:
            w, g = values(rng, n), values(rng, n)
        rows.append(Row(w, None if grad is None else g, wo, (wo + 2) % 4 if grad == "other" else wo, decay))
    return tuple(rows)


# ----------------------------------------------------------------------------- C. one row past 2^32 bytes, tiled
C_PERIODS = 2 ** 18                                                  # pattern blocks: 2^30 floats, 2^32 bytes
C_TAIL = 3 * BLOCK + 5
C_COUNT = C_PERIODS * BLOCK + C_TAIL
C_NEED = 2 * 4 * C_COUNT                                             # w and grad; outputs and workspace are some 20 MB
C_FLOOR = 12 * GIB
# tail indices of the planted values: (NaN, -inf, minimum, maximum) of w and of grad; every one at least 1, so past byte 2^32
C_PLANTED = {"w": (17, BLOCK + 3, 2 * BLOCK + 9, C_TAIL - 1), "g": (BLOCK + 900, 5, C_TAIL - 2, 2 * BLOCK + 77)}


@functools.lru_cache(maxsize=None)
def case_c():
    """(pattern of w [4096], tail of w, pattern of grad, tail of grad): the row is the pattern C_PERIODS times, then the tail."""
    rng = np.random.default_rng(71)
    pw, tw, pg, tg = values(rng, BLOCK), values(rng, C_TAIL), values(rng, BLOCK), values(rng, C_TAIL)
    for tail, key, big in ((tw, "w", A_EXTREME[0]), (tg, "g", A_EXTREME[1])):
        at = C_PLANTED[key]
        tail[list(at)] = [np.nan, -np.inf, -big, big]
    return pw, tw, pg, tg


def tiled_row(pattern, tail, periods):
    return np.concatenate([np.tile(pattern, periods), tail])


def _sequential(pattern_partial, periods, tail_partials):
    """Stage 2 on a row of `periods` equal blocks and a tail: the partials added one by one in block order from +0.0."""
    seq = np.concatenate([[0.0], np.full(periods, pattern_partial, f64), np.asarray(tail_partials, f64)])
    return np.add.accumulate(seq)[-1]


def _partials(d):
    """Stage 1 on whole and trailing blocks of doubles that start on a block boundary."""
    blocks = nref.n_blocks(d.size, 0)
    virt = np.zeros(blocks * BLOCK, f64)
    virt[:d.size] = d
    return nref.block_partials(virt)


def tiled_norm(pattern, tail, periods):
    """tensor_norm of tiled_row(pattern, tail, periods) at pad 0 from the two distinct block contents."""
    sq, bad = nref.squares(np.concatenate([pattern, tail]), 0, 1 + nref.n_blocks(len(tail), 0))
    p = nref.block_partials(sq)
    return _sequential(p[0], periods, p[1:]), periods * int(bad[:BLOCK].sum()) + int(bad[BLOCK:].sum())


def tiled_norms(pw, tw, pg, tg, periods):
    """table_norms of the one-row table -> sums [1,2], bad [1,2]."""
    sums, bad = np.zeros((1, 2), f64), np.zeros((1, 2), np.int64)
    sums[0, 0], bad[0, 0] = tiled_norm(pw, tw, periods)
    sums[0, 1], bad[0, 1] = tiled_norm(pg, tg, periods)
    return sums, bad


def tiled_plane(pattern, tail, periods):
    """histogram_ref.plane of tiled_row(pattern, tail, periods) at pad 0: counts as periods * counts(pattern) + counts(tail), the
    extremes from one pattern and the tail, the sums block by block."""
    cp, sp = href.plane(pattern, 0)
    ct, st = href.plane(tail, 0)
    _c, both = href.plane(np.concatenate([pattern, tail]), 0)
    out = np.zeros((), href.STATS_DTYPE)
    out["num"], out["bad"] = periods * int(sp["num"]) + int(st["num"]), periods * int(sp["bad"]) + int(st["bad"])
    out["min"], out["max"] = both["min"], both["max"]
    x = np.concatenate([pattern, tail])
    d = np.where(np.isfinite(x), x, f32(0)).astype(f64)
    p = _partials(d)
    out["sum"] = _sequential(p[0], periods, p[1:])
    p = _partials(d * d)
    out["sum_squares"] = _sequential(p[0], periods, p[1:])
    return periods * cp + ct, out


def tiled_histograms(pw, tw, pg, tg, decay, weight_decay, periods):
    """table_histograms of the one-row table -> counts [1,2,NB], stats [1,2]."""
    counts, stats = np.zeros((1, 2, href.NB), np.int64), np.zeros((1, 2), href.STATS_DTYPE)
    counts[0, 0], stats[0, 0] = tiled_plane(pw, tw, periods)
    counts[0, 1], stats[0, 1] = tiled_plane(href.gradient_plane(pw, pg, decay, weight_decay), href.gradient_plane(tw, tg, decay, weight_decay),
                                            periods)
    return counts, stats


# ----------------------------------------------------------------------------- D2. many small rows
D2_ROWS = 1500
D2_G = 3
_FIT = {4: 3, 8: 7, 12: 9}                                           # the count that fills so many bucket floats


@functools.lru_cache(maxsize=None)
def d2_table():
    """(counts, kinds, present, marks): counts of 0..9, about one in eight empty, with runs of three empty rows at the start, at bucket
    float 4096 (a row ends there, the next non-empty one starts there) and at the end; a 7-element row at bucket float 8188 that
    crosses into block 2; every tenth row NULL, but not the rows on the two block boundaries; kind 1 on every seventh present row.
    marks: the indices of the row that ends block 0, of the first empty row behind it and of the row that crosses into block 2."""
    rng = np.random.default_rng(81)
    counts, cursor = [0, 0, 0], 0

    def add(n):
        nonlocal cursor
        counts.append(n)
        cursor += -(-n // 4) * 4

    def fill_to(target):
        while cursor + 12 < target:
            add(0 if rng.random() < 0.125 else int(rng.integers(1, 10)))
        if cursor < target:
            add(_FIT[target - cursor])
        assert cursor == target

    add(int(rng.integers(1, 10)))
    fill_to(BLOCK)
    marks = {"ends_block_0": len(counts) - 1, "empty_at_4096": len(counts)}
    counts += [0, 0, 0]
    add(int(rng.integers(1, 10)))
    fill_to(2 * BLOCK - 4)
    marks["crosses_into_block_2"] = len(counts)
    add(7)
    while len(counts) < D2_ROWS - 4:
        add(0 if rng.random() < 0.125 else int(rng.integers(1, 10)))
    add(int(rng.integers(1, 10)))
    counts += [0, 0, 0]
    keep = (marks["ends_block_0"], marks["empty_at_4096"] + 3, marks["crosses_into_block_2"])
    present = [0 if t % 10 == 9 and t not in keep else 1 for t in range(len(counts))]
    kinds, seen = [], 0
    for t in range(len(counts)):
        kinds.append(1 if present[t] and seen % 7 == 6 else 0)
        seen += present[t]
    return tuple(counts), tuple(kinds), tuple(present), marks


def d2_values(rng, counts, kinds, present, G):
    """x[r][t] over +-40 binades (kind 1: moderate, as test_gpu_train_reduce._values draws them), and on the first rows that can hold
    them: -0.0 on every rank, a NaN with a payload on the last rank alone, +inf on every rank, +inf and -inf on two ranks (a created
    NaN), each on a row's last element."""
    x = [[(rng.standard_normal(n) * np.exp2(rng.uniform(-40, 40, n))).astype(f32) for n in counts] for _ in range(G)]
    for r in range(G):
        for t, n in enumerate(counts):
            if kinds[t] == 1:
                x[r][t][:] = np.abs(x[r][t]) % f32(1e6)
    plain = [t for t, n in enumerate(counts) if n >= 2 and kinds[t] == 0 and present[t]]
    stats = [t for t, n in enumerate(counts) if n >= 2 and kinds[t] == 1]
    a, b, c, d = plain[5], plain[len(plain) // 2], plain[-7], plain[-2]
    for r in range(G):
        x[r][a][-1] = f32(-0.0)
        x[r][c][-1] = f32(np.inf)
    x[G - 1][b][-1] = nan(0x12345)
    x[0][d][-1], x[1][d][-1] = f32(np.inf), f32(-np.inf)
    x[G - 1][stats[3]][-1] = nan(0x00042)
    return x, {"neg_zero": a, "nan": b, "inf": c, "created": d, "nan_kind1": stats[3]}


# ----------------------------------------------------------------------------- D3. slices past 2^32 bytes
D3_G = 2
D3_PERIODS = 2 ** 18
D3_TAIL = BLOCK + 5
D3_FRONT = 3                                                         # a 3-float row first: the big row starts at bucket float 4
D3_NEED = 16 * GIB                                                   # two inputs, then the output in their place, and the gathered buffer
D3_FLOOR = 20 * GIB
D3_HEAD = rref.HEADER_FLOATS + 4                                     # slice floats in front of the big row
D3_NAN_AT, D3_INF_AT = 77, BLOCK + 3                                 # tail indices: a NaN with a payload on rank 1; +inf / -inf


def d3_counts(periods):
    return (D3_FRONT, periods * BLOCK + D3_TAIL)


@functools.lru_cache(maxsize=None)
def case_d3():
    """Per rank (the 3-float row, the pattern [4096], the tail): two different patterns."""
    rng = np.random.default_rng(91)
    ranks = []
    for r in range(D3_G):
        front, pattern, tail = [(rng.standard_normal(n) * np.exp2(rng.uniform(-40, 40, n))).astype(f32) for n in (D3_FRONT, BLOCK, D3_TAIL)]
        tail[D3_INF_AT] = f32(np.inf) if r == 0 else f32(-np.inf)
        if r == 1:
            tail[D3_NAN_AT] = nan(0x54321)
        ranks.append((front, pattern, tail))
    return tuple(ranks)


def d3_tiled_pack(front, pattern, tail, header):
    """One rank's slice in three pieces from the slice of the TWO-period row: (the head: header, front row and its padding; one
    period; everything behind the last period: the tail and the +0.0 up to the slice's end).  The rest's length does not depend on
    the periods: 4 + periods * 4096 + 4104 payload floats round up to (periods + 2) * 4096."""
    two = rref.pack_ref([front, tiled_row(pattern, tail, 2)], d3_counts(2), header)
    period = two[D3_HEAD:D3_HEAD + BLOCK]
    assert np.array_equal(period.view(np.uint32), two[D3_HEAD + BLOCK:D3_HEAD + 2 * BLOCK].view(np.uint32))
    return two[:D3_HEAD], period, two[D3_HEAD + 2 * BLOCK:]


def d3_tiled_reduce(big_row_of_two, periods):
    """The reduced big row of `periods` periods from the reduced row of two: its first period repeated, then its tail."""
    two = np.asarray(big_row_of_two, f32)
    assert np.array_equal(two[:BLOCK].view(np.uint32), two[BLOCK:2 * BLOCK].view(np.uint32))
    return np.concatenate([np.tile(two[:BLOCK], periods), two[2 * BLOCK:]])
