"""Tiled detection on the GPU (include/ssd_hip.h, block "tiled detection"): ssd_tile_gather against numpy slicing between guard
words at every source alignment, ssd_tile_merge against tests/helpers/tile_ref.py on the detector's own records and on hand-built
ones through the bare ABI, and Detector.detect_tiled against the hand-made path (numpy crops, detect_batch, the reference merge)."""
import ctypes

import numpy as np
import pytest

from conftest import TINY_PARAMS
from helpers import guarded
from helpers import tile_ref as ref

pytestmark = pytest.mark.gpu

TILE, OVERLAP = 128, 0.25
FRAME = (200, 301)                          # six tiles per frame: rows 0, 72, columns 0, 96, 173
C, M = TINY_PARAMS["num_classes"], TINY_PARAMS["max_boxes_per_class"]
THR = TINY_PARAMS["iou_threshold"]


def stream_ptr(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("layout", ["aligned", "skewed"])
@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("frame", [(200, 301), (129, 131), (300, 128)])
def test_gather_equals_numpy_slicing_at_every_source_alignment(ssd, cuda, frame, F, layout):
    H, W = frame
    frames = np.random.default_rng(H * W + F).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    want = ref.crops(frames, TILE, TILE, OVERLAP)
    ys, xs = ssd.tile_grid(H, W, TILE, TILE, OVERLAP)
    assert want.shape[0] == F * len(ys) * len(xs)
    if frame == (129, 131):
        assert (ys, xs) == ([0, 1], [0, 3])                   # four almost coincident tiles
    oy, ox = ssd.tiles.overlap_pixels(TILE, TILE, OVERLAP)
    starts = set()
    for k in range(4):                                        # frames_dev = a 4-byte aligned base + k
        arena = guarded.Arena(cuda, "cuda:0", layout)
        block = np.concatenate([np.full(k, 0x5A, np.uint8), frames.reshape(-1)])
        arena.add("frames", block, np.uint8, 4, "input")
        arena.add("tiles", want.shape, np.uint8, 4, "output", fill=0xA5)
        src = arena.ptr("frames") + k
        assert (src - k) % 4 == 0
        for f in range(F):
            for y0 in ys:
                for x0 in xs:
                    starts |= {(src + ((f * H + y0 + y) * W + x0) * 3) % 4 for y in range(TILE)}
        ssd._lib.check(ssd.lib().ssd_tile_gather(src, F, H, W, TILE, TILE, oy, ox, arena.ptr("tiles"), stream_ptr(cuda)))
        cuda.cuda.synchronize()
        assert np.array_equal(arena.read("tiles"), want), k
        arena.check()                                         # guards and the input (its k leading bytes too) intact
        if W % 4:
            assert starts == {0, 1, 2, 3}                     # an odd row pitch meets every offset in ONE call
    assert starts == {0, 1, 2, 3}


# ----------------------------------------------------------------------------- the detector's own records
@pytest.fixture(scope="module")
def detector(ssd, cuda):
    W = ssd.synthetic_weights(TINY_PARAMS, seed=1, logits_bias=-3.0)
    det = ssd.Detector(W, config=dict(TINY_PARAMS))
    yield det
    det.close()


@pytest.fixture(scope="module")
def real(ssd, cuda, detector, oracle_ops):
    """Two different 200 x 301 frames through the engine: the tiles' records from the device gather, the records of the numpy
    crops, the whole frames' records, and the reference merge with and without the latter"""
    H, W = FRAME
    rng = np.random.default_rng(5)
    # blocks of 8 x 8 pixels of one colour: structure at the scale of the smallest anchors, the same in neighbouring tiles
    coarse = rng.integers(0, 256, (2, H // 8 + 1, W // 8 + 1, 3), dtype=np.uint8)
    frames = np.ascontiguousarray(np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :H, :W])
    eng = detector.engine
    dev = cuda.from_numpy(frames).cuda()
    tiles = ssd.tiles.tile_gather(dev, TILE, TILE, OVERLAP)
    n = tiles.shape[0]
    rec = eng.new_records(n, "cuda:0")
    eng.forward(tiles[:8], records=rec[:8])
    eng.forward(tiles[8:], records=rec[8:])
    rec_crops = eng.new_records(n, "cuda:0")
    crops = cuda.from_numpy(ref.crops(frames, TILE, TILE, OVERLAP)).cuda()
    eng.forward(crops[:8], records=rec_crops[:8])
    eng.forward(crops[8:], records=rec_crops[8:])
    rec_full = eng.new_records(2, "cuda:0")
    eng.forward(dev, records=rec_full)
    cuda.cuda.synchronize()
    geo = (2, H, W, TILE, TILE, OVERLAP, C, M, THR)
    t, fl = rec.cpu().numpy(), rec_full.cpu().numpy()
    return {"frames": frames, "rec": rec, "rec_crops": rec_crops, "rec_full": rec_full, "geo": geo,
            "want_full": ref.merge(oracle_ops, t, fl, *geo), "want_tiles": ref.merge(oracle_ops, t, None, *geo),
            "stats": ref.cross_source_stats(t, fl, *geo)}


def test_the_tiles_path_adds_nothing(real):
    assert real["rec"].shape == (12, 6 * C * M + 1)
    assert np.array_equal(real["rec"].cpu().numpy(), real["rec_crops"].cpu().numpy())
    assert ref.split(real["rec"].cpu().numpy())[3].sum() > 0


@pytest.mark.parametrize("full", [True, False])
def test_merge_of_real_records_equals_the_reference(ssd, cuda, real, full):
    got = ssd.tiles.tile_merge(real["rec"], real["rec_full"] if full else None, (2,) + FRAME, TILE, TILE, OVERLAP, C, M, THR)
    want = real["want_full" if full else "want_tiles"]
    assert np.array_equal(got.cpu().numpy(), want)
    cross, most = real["stats"]
    print("suppressions across tiles %d, most sources of one class %d, boxes %s" % (cross, most, ref.split(want)[3]))
    assert cross >= 1                       # a box of one tile suppressed by a box of another
    assert most >= 3                        # a class with candidates from three or more sources
    assert not np.array_equal(want[0], want[1])


# ----------------------------------------------------------------------------- hand-built records through the bare ABI
HC, HM = 3, 4                               # classes, boxes per class of the hand-built cases
HT = HC * HM


def tile_box(frame_box, y0, x0, H=FRAME[0], W=FRAME[1]):
    """a box in frame-normalised coordinates, as tile (y0, x0) reports it"""
    b = np.asarray(frame_box, np.float64)
    return ((b[0] * H - y0) / TILE, (b[1] * W - x0) / TILE, (b[2] * H - y0) / TILE, (b[3] * W - x0) / TILE)


def hand_cases():
    """name -> (tile rows [F * 6 records], full rows [F records] or None, F, iou threshold).  Tiles of a 200 x 301 frame: index
    (iy * 3 + ix) at rows (0, 72) x columns (0, 96, 173)."""
    empty = [[] for _ in range(6)]
    obj = (0.45, 0.40, 0.60, 0.52)          # inside tile 1 (0, 96) and tile 4 (72, 96)
    cases = {}

    def two_tiles(s1, s4):
        rows = [list(r) for r in empty]
        rows[1] = [(1, s1, tile_box(obj, 0, 96))]
        rows[4] = [(1, s4, tile_box(obj, 72, 96))]
        return rows
    cases["same object, higher score in the later tile"] = (two_tiles(0.5, 0.7), None, 1, 0.5)
    cases["same object, equal scores"] = (two_tiles(0.6, 0.6), None, 1, 0.5)
    # whole-frame rows pass bit for bit: IoU of these two is exactly 0.125 / 0.25 = 0.5
    a, b = (0.0, 0.0, 0.5, 0.5), (0.0, 0.0, 0.5, 0.25)
    cases["IoU exactly at the threshold"] = (empty, [[(0, 0.9, a), (0, 0.8, b)]], 1, 0.5)
    cases["IoU just above the threshold"] = (empty, [[(0, 0.9, a), (0, 0.8, b)]], 1, float(np.nextafter(np.float32(0.5), np.float32(0))))
    flat, point = (0.2, 0.2, 0.2, 0.6), (0.3, 0.3, 0.3, 0.3)
    cases["zero-area boxes"] = (empty, [[(2, 0.9, a), (2, 0.8, flat), (2, 0.7, a), (2, 0.6, flat), (2, 0.5, point)]], 1, 0.5)
    many = [list(r) for r in empty]
    for s in range(6):                      # disjoint small boxes: 12 survivors of class 0, truncated at HM
        many[s] = [(0, 0.3 + 0.05 * s + 0.01 * k, (0.1 * k, 0.1 * k, 0.1 * k + 0.05, 0.1 * k + 0.05)) for k in range(2)]
    cases["more than m survivors"] = (many, None, 1, 0.5)
    cases["sources without boxes"] = ([[], [(1, 0.5, (0.1, 0.1, 0.4, 0.4))], [], [], [(2, 0.4, (0.5, 0.5, 0.9, 0.9))], []], [[]], 1, 0.5)
    cases["all sources empty"] = (empty, [[]], 1, 0.5)
    cases["all sources empty, no whole frame"] = (empty, None, 1, 0.5)
    f0 = two_tiles(0.5, 0.7)
    f1 = [list(r) for r in many]
    f1[3].append((2, 0.9, (0.2, 0.2, 0.8, 0.8)))
    cases["two frames"] = (f0 + f1, [[(1, 0.8, obj), (0, 0.4, a)], [(2, 0.95, (0.25, 0.25, 0.8, 0.8))]], 2, 0.5)
    return cases


HAND = hand_cases()


def run_merge(ssd, cuda, tile_rec, full_rec, F, thr, H=FRAME[0], W=FRAME[1], o=32, Cn=HC, m=HM, stream=None):
    """-> (the output records, the arena): NaN-filled output and the inputs between guard words"""
    arena = guarded.Arena(cuda, "cuda:0", "skewed")
    arena.add("tile_rec", tile_rec, np.int32, 4, "input")
    if full_rec is not None:
        arena.add("full_rec", full_rec, np.int32, 4, "input")
    arena.add("out", (F, 6 * Cn * m + 1), np.int32, 4, "output")
    arena.view("out")
    cuda.cuda.synchronize()
    with cuda.cuda.stream(stream if stream is not None else cuda.cuda.current_stream()):
        ssd._lib.check(ssd.lib().ssd_tile_merge(arena.ptr("tile_rec"), arena.ptr("full_rec" if full_rec is not None else None), F, H, W,
                                                TILE, TILE, o, o, Cn, m, thr, arena.ptr("out"), stream_ptr(cuda)))
    cuda.cuda.synchronize()
    return arena.read("out"), arena


@pytest.mark.parametrize("name", list(HAND))
def test_merge_of_hand_built_records(ssd, cuda, oracle_ops, name):
    tile_rows, full_rows, F, thr = HAND[name]
    tile_rec = ref.records(tile_rows, HT)
    full_rec = None if full_rows is None else ref.records(full_rows, HT)
    want = ref.merge(oracle_ops, tile_rec, full_rec, F, *FRAME, TILE, TILE, OVERLAP, HC, HM, thr)
    got, arena = run_merge(ssd, cuda, tile_rec, full_rec, F, thr)
    assert np.array_equal(got, want)                                                      # every word written: none kept the NaN fill
    arena.check()                                                                         # none outside, inputs intact
    boxes, labels, scores, num = ref.split(got)
    f32 = np.float32
    if name.startswith("same object"):
        assert num[0] == 1 and labels[0, 0] == 1
        later = name.endswith("later tile")
        assert scores[0, 0] == f32(0.7 if later else 0.6)
        src = (72, 96) if later else (0, 96)            # equal scores: the lower source survives
        assert np.array_equal(boxes[0, :1], ref.to_frame(ref.split(tile_rec)[0][4 if later else 1, :1], *src, TILE, TILE, *FRAME))
    elif name == "IoU exactly at the threshold":
        assert num[0] == 2                              # the comparison is a strict >
        assert np.array_equal(got[0, :8], full_rec[0, :8])                                # whole-frame rows bit for bit
    elif name == "IoU just above the threshold":
        assert num[0] == 1
    elif name == "zero-area boxes":
        assert num[0] == 4 and list(scores[0, :4]) == [f32(0.9), f32(0.8), f32(0.6), f32(0.5)]    # only the repeat of `a` goes
    elif name == "more than m survivors":
        assert num[0] == HM and np.all(labels[0, :HM] == 0) and scores[0, 0] == f32(0.3 + 0.05 * 5 + 0.01)
    elif name == "sources without boxes":
        assert num[0] == 2 and list(labels[0, :2]) == [1, 2]
    elif name.startswith("all sources empty"):
        assert not got.any()
    elif name == "two frames":
        assert num[0] == 2 and num[1] == HM + 2 and not np.array_equal(got[0], got[1])


def test_merge_on_a_side_stream_and_again_gives_the_same_bits(ssd, cuda):
    tile_rows, full_rows, F, thr = HAND["two frames"]
    tile_rec, full_rec = ref.records(tile_rows, HT), ref.records(full_rows, HT)
    first, _ = run_merge(ssd, cuda, tile_rec, full_rec, F, thr)
    side, arena = run_merge(ssd, cuda, tile_rec, full_rec, F, thr, stream=cuda.cuda.Stream())
    arena.check()
    again, _ = run_merge(ssd, cuda, tile_rec, full_rec, F, thr)
    assert np.array_equal(first, side) and np.array_equal(first, again)


def test_merge_at_the_candidate_cap(ssd, cuda, oracle_ops):
    """(ny * nx + 1) * m == SSD_TILE_MAX_CANDIDATES: a one-row frame of 511 tiles, every source with m boxes of one class -- all
    2048 candidates of the class in LDS -- and the call one tile wider is refused"""
    cap, m = ssd.tiles.MAX_CANDIDATES, 4
    nx = cap // m - 1
    rng = np.random.default_rng(3)
    rows = [[(0, float(rng.choice([0.3, 0.5, 0.7])), (0.1 * k, 0.2, 0.1 * k + 0.3, 0.9)) for k in range(m)] for _ in range(nx)]
    tile_rec = ref.records(rows, m)
    full_rec = ref.records([[(0, 0.6, (0.0, 0.001 * k, 1.0, 0.001 * k + 0.002)) for k in range(m)]], m)
    H, W = TILE, TILE * nx
    want = ref.merge(oracle_ops, tile_rec, full_rec, 1, H, W, TILE, TILE, 0.0, 1, m, 0.5)
    got, arena = run_merge(ssd, cuda, tile_rec, full_rec, 1, 0.5, H=H, W=W, o=0, Cn=1, m=m)
    assert np.array_equal(got, want) and ref.split(got)[3][0] == m
    arena.check()
    with pytest.raises(ssd.SsdError, match="exceed SSD_TILE_MAX_CANDIDATES"):
        run_merge(ssd, cuda, np.concatenate([tile_rec, tile_rec[:1]]), full_rec, 1, 0.5, H=H, W=W + TILE, o=0, Cn=1, m=m)


# ----------------------------------------------------------------------------- end to end
def by_hand(detector, oracle_ops, frame, full_frame, score_threshold):
    """the parent's API: numpy crops, detect_batch, the reference merge, the score filter"""
    from ssd_amd.ssd import pack_records, score_filter
    H, W, _ = frame.shape
    tile_rec = pack_records(*detector.detect_batch(ref.crops(frame[None], TILE, TILE, OVERLAP)))
    full_rec = pack_records(*detector.detect_batch(frame[None])) if full_frame else None
    boxes, labels, scores, num = ref.split(ref.merge(oracle_ops, tile_rec, full_rec, 1, H, W, TILE, TILE, OVERLAP, C, M, THR))
    return score_filter(boxes[0], labels[0], scores[0], num[0], score_threshold)


@pytest.mark.parametrize("full_frame", [True, False])
def test_detect_tiled_equals_the_hand_made_path(cuda, detector, oracle_ops, real, full_frame):
    frame = real["frames"][0]
    detector.detect_tiled(frame, full_frame=full_frame)                  # (builds what plans it needs)
    misses = detector.engine.plan_cache_stats()["misses"]
    got = detector.detect_tiled(frame, full_frame=full_frame)
    assert detector.engine.plan_cache_stats()["misses"] == misses        # a second call builds no new plan
    want = by_hand(detector, oracle_ops, frame, full_frame, 0.1)
    assert len(want[2]) > 0
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    dev = detector.detect_tiled(cuda.from_numpy(frame).cuda(), full_frame=full_frame)
    for g, w in zip(dev, got):
        assert np.array_equal(g, w)                                      # host input and CUDA input: the same result
    # closed under score_threshold: a higher threshold returns exactly the rows above it, in order
    cut = float(np.median(got[2]))
    fewer = detector.detect_tiled(frame, full_frame=full_frame, score_threshold=cut)
    keep = got[2] > cut
    assert 0 < keep.sum() < len(keep)
    for g, w in zip(fewer, got):
        assert np.array_equal(g, w[keep])


def test_detect_tiled_on_a_batch_of_frames_and_its_refusals(detector, real):
    both = detector.detect_tiled(real["frames"], max_batch=4)            # 12 tiles as 4 + 4 + 4
    assert isinstance(both, list) and len(both) == 2
    for f in range(2):
        one = detector.detect_tiled(real["frames"][f])
        for g, w in zip(both[f], one):
            assert np.array_equal(g, w)
    with pytest.raises(ValueError, match="use __call__"):
        detector.detect_tiled(np.zeros((100, 301, 3), np.uint8))
    with pytest.raises(ValueError, match="min_dimension"):
        detector.detect_tiled(real["frames"][0], tile=256)
    with pytest.raises(ValueError, match="uint8"):
        detector.detect_tiled(real["frames"][0].astype(np.float32))
