"""Tiled detection without a GPU (include/ssd_hip.h, block "tiled detection"): the grid, the reference merge of
tests/helpers/tile_ref.py against its brute-force restatement, and every refusal of the entry points, which come before any HIP
call."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import tile_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("frame,tile,ys,xs", [((1200, 1600), 640, [0, 480, 560], [0, 480, 960]),
                                              ((200, 301), 128, [0, 72], [0, 96, 173])])
def test_grid_known_answers(ssd, frame, tile, ys, xs):
    assert ssd.tile_grid(frame[0], frame[1], tile, tile, 0.25) == (ys, xs)
    assert ref.grid(frame[0], frame[1], tile, tile, 0.25) == (ys, xs)
    assert len(ys) * len(xs) == {640: 9, 128: 6}[tile]


def test_grid_a_frame_as_high_as_the_tile_has_one_row(ssd):
    assert ssd.tile_grid(128, 500, 128, 128, 0.25) == ([0], [0, 96, 192, 288, 372])
    assert ssd.tile_grid(128, 128, 128, 128, 0.25) == ([0], [0])
    assert ssd.tile_grid(256, 640, 128, 256, 0.0) == ([0, 128], [0, 256, 384])


def test_grid_covers_every_pixel_and_repeats_no_tile(ssd):
    rng = np.random.default_rng(11)
    for _ in range(300):
        th, tw = (int(v) * 128 for v in rng.integers(1, 4, 2))
        H, W = th + int(rng.integers(0, 700)), tw + int(rng.integers(0, 700))
        overlap = float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.9, 0.99]))
        ys, xs = ssd.tile_grid(H, W, th, tw, overlap)
        assert (ys, xs) == ref.grid(H, W, th, tw, overlap), (H, W, th, tw, overlap)
        for origins, side, full in ((ys, th, H), (xs, tw, W)):
            assert origins[0] == 0 and origins[-1] == full - side
            assert all(b > a for a, b in zip(origins, origins[1:]))                 # strictly increasing: no duplicate tile
            assert all(b <= a + side for a, b in zip(origins, origins[1:]))         # no gap: every pixel lies in a tile
            seen = np.zeros(full, bool)
            for o in origins:
                seen[o:o + side] = True
            assert seen.all()


def test_grid_refusals_are_value_errors(ssd):
    for args, word in (((127, 300, 128, 128, 0.25), "H is below th"), ((300, 127, 128, 128, 0.25), "W is below tw"),
                       ((300, 300, 100, 128, 0.25), "th must be a positive multiple of 128"),
                       ((300, 300, 128, 192, 0.25), "tw must be a positive multiple of 128"),
                       ((300, 300, 128, 128, 1.0), "step th - oy below 1"), ((300, 300, 128, 128, -0.5), "oy must not be negative")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ssd.tile_grid(*args)


def test_python_constant_is_the_headers(ssd):
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    cap = int(re.search(r"#define SSD_TILE_MAX_CANDIDATES (\d+)", hdr).group(1))
    assert ssd.tiles.MAX_CANDIDATES == cap and cap >= 1024


# ----------------------------------------------------------------------------- the reference merge, twice
def random_records(rng, F, C, m, H, W, th, tw, origins, full):
    """Records of at most m rows per class, class-major like the detector's.  A frame has a pool of objects on a coarse pixel
    lattice (plenty of overlaps, exact repeats and zero-area boxes) with scores from a few values (plenty of ties); a tile reports,
    in its own coordinates, some of the objects that lie inside it -- so neighbouring tiles report the same object -- and the
    whole frame's record some of all.  origins: (ys, xs) of the tiles."""
    ys, xs = origins
    per = []
    for _f in range(F):
        pool = []
        for _k in range(40):
            y0, x0 = int(rng.integers(0, H // 16)) * 16, int(rng.integers(0, W // 16)) * 16
            h, w = int(rng.integers(0, 5)) * 16, int(rng.integers(0, 5)) * 16
            pool.append((int(rng.integers(0, C)), float(rng.choice([0.2, 0.35, 0.5, 0.5, 0.8])), (y0, x0, min(y0 + h, H), min(x0 + w, W))))
        for oy, ox, sh, sw in ([(0, 0, H, W)] if full else [(y, x, th, tw) for y in ys for x in xs]):
            rows = []
            for c in range(C):
                inside = [(lb, sc, ((b[0] - oy) / sh, (b[1] - ox) / sw, (b[2] - oy) / sh, (b[3] - ox) / sw)) for lb, sc, b in pool
                          if lb == c and b[0] >= oy and b[1] >= ox and b[2] <= oy + sh and b[3] <= ox + sw and rng.random() < 0.8]
                rows += inside[:m]
            per.append(rows)
    return ref.records(per, C * m)


GEOMETRY = (200, 301, 128, 128, 0.25)      # H, W, th, tw, overlap: six tiles
C, M, F = 3, 4, 2


@pytest.fixture(scope="module")
def cases(ssd):
    """The tiles report their objects at the origins the LIBRARY gives (ssd.tile_grid); the reference merge moves them back with
    its own restatement of the grid, so the two statements of the grid meet in every case below."""
    origins = ssd.tile_grid(*GEOMETRY)
    assert origins == ref.grid(*GEOMETRY) == ([0, 72], [0, 96, 173])
    geo = GEOMETRY[:4] + (origins,)
    out = []
    for seed in range(6):
        rng = np.random.default_rng(seed)
        tile_rec = random_records(rng, F, C, M, *geo, False)
        full_rec = random_records(rng, F, C, M, *geo, True) if seed % 2 == 0 else None
        assert tile_rec.shape[0] == F * 6
        out.append((tile_rec, full_rec, [0.5, 0.6, 0.3][seed % 3]))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_merge_equals_its_brute_force_restatement(oracle_ops, cases, seed):
    tile_rec, full_rec, thr = cases[seed]
    a = ref.merge(oracle_ops, tile_rec, full_rec, F, *GEOMETRY, C, M, thr)
    b = ref.merge_brute(tile_rec, full_rec, F, *GEOMETRY, C, M, thr)
    assert np.array_equal(a, b)
    boxes, labels, scores, num = ref.split(a)
    assert num.min() > 0 and num.max() <= C * M
    for f in range(F):
        n = int(num[f])
        assert np.all(np.diff(labels[f, :n]) >= 0)                                          # classes ascending
        assert not boxes[f, n:].any() and not scores[f, n:].any() and not labels[f, n:].any()
        for c in range(C):
            assert np.all(np.diff(scores[f, :n][labels[f, :n] == c]) <= 0) and (labels[f, :n] == c).sum() <= M


def test_those_records_suppress_across_tiles_and_draw_on_many_sources(cases):
    """What makes the six cases above worth running: boxes of one tile are suppressed by boxes of another, and a class draws its
    candidates from many sources -- records that never met across tiles would agree in both restatements whatever the order."""
    stats = [ref.cross_source_stats(t, fr, F, *GEOMETRY, C, M, thr) for t, fr, thr in cases]
    assert sum(c for c, _ in stats) >= 6 and max(m for _, m in stats) >= 5, stats


def test_the_fp32_move_is_one_operation_at_a_time(ssd):
    """The reference's move of a box from the library's last tile (ssd.tile_grid's last origins) to the frame rounds after every
    operation, as the header demands of the kernel: what the GPU tests compare the merge with is that and not a float64 formula."""
    ys, xs = ssd.tile_grid(*GEOMETRY)
    assert (ys[-1], xs[-1]) == (72, 173)
    b = np.array([[0.1, 0.7, 0.9, 0.3]], np.float32)
    got = ref.to_frame(b, ys[-1], xs[-1], 128, 128, 200, 301)
    want = [np.float32(np.float32(np.float32(v * np.float32(128)) + np.float32(o)) / np.float32(n))
            for v, o, n in zip(b[0], (72, 173, 72, 173), (200, 301, 200, 301))]
    assert got.dtype == np.float32 and np.array_equal(got[0], np.array(want, np.float32))
    # ... which is not what one float64 evaluation rounds to for every input: the order of roundings is part of the contract
    x = np.random.default_rng(0).random(4096).astype(np.float32)
    one = ((x * np.float32(128)) + np.float32(173)) / np.float32(301)
    assert np.any(one != ((x.astype(np.float64) * 128 + 173) / 301).astype(np.float32))


# ----------------------------------------------------------------------------- refusals
def test_the_entry_points_refuse_before_any_hip_call(ssd):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the call
    never reads."""
    lib = ssd.lib()
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    cap = ssd.tiles.MAX_CANDIDATES

    def gather(frames=fake, tiles=fake, F=1, H=200, W=301, th=128, tw=128, oy=32, ox=32):
        rc = lib.ssd_tile_gather(frames, F, H, W, th, tw, oy, ox, tiles, None)
        return rc, lib.ssd_last_error().decode()

    def merge(tile_rec=fake, full=fake, out=fake, F=1, H=200, W=301, th=128, tw=128, oy=32, ox=32, C=3, m=4, thr=0.5):
        rc = lib.ssd_tile_merge(tile_rec, full, F, H, W, th, tw, oy, ox, C, m, thr, out, None)
        return rc, lib.ssd_last_error().decode()

    def refused(fn, word, **kw):
        rc, msg = fn(**kw)
        assert rc == -1 and msg.startswith("ssd_tile_%s: " % fn.__name__) and word in msg, (rc, msg)

    refused(gather, "frames_dev is NULL", frames=None)
    refused(gather, "tiles_dev is NULL", tiles=None)
    for k in (1, 2, 3):
        refused(gather, "tiles_dev must be 4-byte aligned", tiles=fake + k)
    refused(merge, "tile_records_dev is NULL", tile_rec=None)
    refused(merge, "out_records_dev is NULL", out=None)
    refused(merge, "tile_records_dev must be 4-byte aligned", tile_rec=fake + 2)
    refused(merge, "full_records_dev must be 4-byte aligned", full=fake + 1)
    refused(merge, "out_records_dev must be 4-byte aligned", out=fake + 3)
    refused(merge, "C must be at least 1", C=0)
    refused(merge, "m must be at least 1", m=0)
    refused(merge, "iou_threshold is NaN", thr=float("nan"))
    for fn in (gather, merge):
        refused(fn, "th must be a positive multiple of 128", th=100)
        refused(fn, "th must be a positive multiple of 128", th=0)
        refused(fn, "tw must be a positive multiple of 128", tw=192)
        refused(fn, "H is below th", H=127)
        refused(fn, "W is below tw", W=127)
        refused(fn, "step th - oy below 1", oy=128)
        refused(fn, "step tw - ox below 1", ox=200)
        refused(fn, "oy must not be negative", oy=-1)
        refused(fn, "F must be at least 1", F=0)
        refused(fn, "must be below 2^31 bytes", F=4, H=16384, W=16384)
    # the candidate cap: (ny * nx + 1) * m candidates of one class, on a one-row frame of nx tiles without overlap.  AT the cap the
    # call gets past the cap's check to the one behind it (C * m, made to fail here: a call that passed every check would go on to
    # the launch, which tests/test_gpu_tiles.py makes); one tile beyond the cap it is refused for the cap
    m = 4
    nx_at_cap = cap // m - 1
    g = (ctypes.c_int32 * 4)()
    assert lib.ssd_tile_grid(128, 128 * nx_at_cap, 128, 128, 0, 0, g) == 0 and (g[0] * g[1] + 1) * m == cap
    refused(merge, "C * m must be at most 2^24", H=128, W=128 * nx_at_cap, oy=0, ox=0, m=m, C=(1 << 24) // m + 1)
    refused(merge, "exceed SSD_TILE_MAX_CANDIDATES (%d)" % cap, H=128, W=128 * (nx_at_cap + 1), oy=0, ox=0, m=m, C=(1 << 24) // m + 1)
    refused(merge, "exceed SSD_TILE_MAX_CANDIDATES (%d)" % cap, H=128, W=128 * (nx_at_cap + 1), oy=0, ox=0, m=m)
    refused(merge, "exceed SSD_TILE_MAX_CANDIDATES (%d)" % cap, H=128, W=128 * (nx_at_cap + 1), oy=0, ox=0, m=m, full=None)
    assert lib.ssd_tile_grid(128, 128, 128, 128, 0, 0, None) == -1 and "grid_out is NULL" in lib.ssd_last_error().decode()
