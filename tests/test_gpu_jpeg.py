"""-m gpu: the JPEG decoder (include/ssd_hip.h, block "the JPEG decoder"; csrc/jpeg.hip, jpeg.py) against the decoder the product
used before, PIL.Image.open(...).convert("RGB"), bit for bit -- the shared case list as one batch and reversed, images past one
grid pass of either launch, the call between guard words at 16-byte-not-32-byte addresses, a side stream, the edge batch sizes,
refused files, and the routes built on it: Detector.detect_many_jpeg, detect_many_records_jpeg, coco_eval.evaluate(jpeg_device=).
Independently of PIL and of any file: ssd_jpeg_decode on synthetic tables and coefficients over its whole input domain (int16
extremes, 16-bit table values: sums that wrap in both passes) against the header's restatement.  And the files of
tests/helpers/jpeg_loud.py at and past the edge of the header's "pinned streams" rule, through the decoder and the detector routes."""
import ctypes
import io
import json
import os
import sys

import numpy as np
import pytest

from tests.helpers import guarded, jpeg_cases, jpeg_loud, jpeg_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = -1, -5
GRID_CAP = 1024                     # SSD_COCO_GRID_CAP: groups of a launch; 32 blocks / 4096 pixels per group and pass


@pytest.fixture(scope="module")
def dec(cuda, ssd):
    return ssd.JpegDecoder(0)


def frames_of(result):
    """decode_many's ((flat, hw, offsets), refused) -> ([uint8 [H, W, 3]...], refused)."""
    (flat, hw, offsets), refused = result
    host = flat.cpu().numpy()
    return [host[o:o + 3 * h * w].reshape(h, w, 3) for (h, w), o in zip(hw, offsets)], refused


def progressive(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", progressive=True, quality=90)
    return buf.getvalue()


def loud(arr):
    """A baseline file whose table values are all 255: ssd_jpeg_info_read accepts it, ssd_jpeg_entropy refuses it."""
    blob, p = bytearray(jpeg_cases.encode(arr, "444", 90)), 2
    while blob[p + 1] != 0xDA:
        n = (blob[p + 2] << 8) | blob[p + 3]
        if blob[p + 1] == 0xDB:
            for q in range(p + 4, p + 2 + n, 65):
                blob[q + 1:q + 65] = b"\xff" * 64
        p += 2 + n
    return bytes(blob)


def test_whole_case_list_as_one_batch_and_reversed(dec):
    blobs = [b for _n, b in jpeg_cases.cases()]
    want = jpeg_cases.expected()
    got, refused = frames_of(dec.decode_many(blobs))
    assert refused == {} and len(got) == len(want) == 432
    bad = [jpeg_cases.cases()[i][0] for i in range(432) if not np.array_equal(got[i], want[i])]
    assert not bad, "%d frames differ from PIL, the first: %s" % (len(bad), bad[:5])
    back, refused = frames_of(dec.decode_many(blobs[::-1]))
    assert refused == {}
    bad = [jpeg_cases.cases()[431 - i][0] for i in range(432) if not np.array_equal(back[i], want[431 - i])]
    assert not bad, "reversed: %d frames differ, the first: %s" % (len(bad), bad[:5])


def test_past_one_grid_pass_of_both_launches(dec):
    """One 480x640 4:2:0 (7200 blocks) and one 427x640 4:2:2 (8640) cannot pass the first launch's 1024 x 32 blocks, nor the
    second's 1024 x 4096 pixels, so the batch holds them three and two times (38 880 blocks: the stride loop of launch 1 runs
    twice) and, for launch 2, the smallest 4:2:0 image that alone exceeds a pass: 2064 x 2040 (4 210 560 pixels, 49 665 blocks)."""
    a = jpeg_cases.encode(jpeg_cases.pixels(480, 640, "ramp", 1), "420", 90)
    b = jpeg_cases.encode(jpeg_cases.pixels(427, 640, "noise", 2), "422", 30)
    big = jpeg_cases.encode(jpeg_cases.pixels(2064, 2040, "ramp", 3), "420", 90)
    blobs = [a, b, a, b, a]
    infos = [dec.read_info(x)[1] for x in blobs]
    assert sum(sum(i.blocks) for i in infos) > GRID_CAP * 32
    got, refused = frames_of(dec.decode_many(blobs))
    assert refused == {}
    for g, blob in zip(got, blobs):
        assert np.array_equal(g, jpeg_cases.pil_rgb(blob))
    info = dec.read_info(big)[1]
    assert info.height * info.width > GRID_CAP * 4096 and sum(info.blocks) > GRID_CAP * 32
    got, refused = frames_of(dec.decode_many([big, a]))
    assert refused == {} and np.array_equal(got[0], jpeg_cases.pil_rgb(big)) and np.array_equal(got[1], jpeg_cases.pil_rgb(a))


def host_batch(ssd, blobs):
    """The host stage by hand: (table, coef int16, quant uint16, totals) of a batch of accepted files."""
    from importlib import import_module
    L, lib = import_module("ssd_amd._lib"), ssd.lib()
    infos = (L.SsdJpegInfo * len(blobs))()
    for k, blob in enumerate(blobs):
        assert lib.ssd_jpeg_info_read(blob, len(blob), ctypes.byref(infos[k])) == 0
    table, totals = (L.SsdJpegImage * len(blobs))(), (ctypes.c_int64 * 4)()
    assert lib.ssd_jpeg_plan(infos, len(blobs), table, totals) == 0
    coef, quant = np.zeros(totals[0], np.int16), np.zeros(totals[1], np.uint16)
    for k, blob in enumerate(blobs):
        assert lib.ssd_jpeg_entropy(blob, len(blob), ctypes.byref(infos[k]), coef.ctypes.data + 2 * table[k].coef_offset,
                                    quant.ctypes.data + 2 * table[k].quant_offset) == 0
    return table, coef, quant, list(totals)


@pytest.mark.parametrize("layout", ["skewed", "aligned"])
def test_between_guard_words_every_frame_byte_written_once(cuda, ssd, layout):
    """Table, coefficients, tables, workspace and frames in ONE arena between guard words (skewed: every base 16 and not 32 bytes
    aligned): every frame byte is written whatever it held before, the bytes between frames keep what they held, no guard changes."""
    picks = list(range(0, 432, 5))                                   # every size, sampling, quality and variant
    blobs = [jpeg_cases.cases()[i][1] for i in picks] + [jpeg_cases.encode(jpeg_cases.pixels(150, 211, "ramp", 9), "420", 90)]
    want = [jpeg_cases.expected()[i] for i in picks] + [jpeg_cases.pil_rgb(blobs[-1])]
    table, coef, quant, totals = host_batch(ssd, blobs)
    ws_bytes = int(ssd.lib().ssd_jpeg_workspace_bytes(table, len(blobs)))
    assert ws_bytes == totals[2] and ssd.lib().ssd_jpeg_workspace_bytes(table, len(blobs) + (1 << 21)) == 0
    inside = np.zeros(totals[3], bool)
    for t in table:
        inside[t.frame_offset:t.frame_offset + 3 * t.height * t.width] = True
    assert (~inside).sum() > 0, "the batch must leave gaps between frames"
    results = []
    for fill in (0x3C, 0xC3):
        arena = guarded.Arena(cuda, "cuda:0", layout)
        arena.add("table", np.frombuffer(bytes(table), np.uint8).copy(), np.uint8, 16, "input")
        arena.add("coef", coef.view(np.uint8), np.uint8, 16, "input")
        arena.add("quant", quant.view(np.uint8), np.uint8, 16, "input")
        arena.add("ws", (ws_bytes,), np.uint8, 16, "workspace")
        arena.add("frames", (totals[3],), np.uint8, 16, "output", fill=fill)
        if layout == "skewed":
            assert all(arena.ptr(n) % 32 == 16 for n in ("table", "coef", "quant", "ws", "frames"))
        ssd._lib.check(ssd.lib().ssd_jpeg_decode(table, arena.ptr("table"), len(blobs), arena.ptr("coef"), arena.ptr("quant"),
                                                 arena.ptr("ws"), arena.ptr("frames"), None))
        cuda.cuda.synchronize()
        arena.check()
        out = arena.read("frames")
        assert np.all(out[~inside] == fill), "a byte between two frames was written"
        for t, w in zip(table, want):
            assert np.array_equal(out[t.frame_offset:t.frame_offset + w.size].reshape(w.shape), w)
        results.append(out[inside])
    assert np.array_equal(results[0], results[1])


def test_side_stream_second_launch_and_edge_batches(cuda, dec):
    blobs = [b for _n, b in jpeg_cases.cases()[::9]]
    first, _ = frames_of(dec.decode_many(blobs))
    side = cuda.cuda.Stream()
    with cuda.cuda.stream(side):
        second = dec.decode_many(blobs)
        third = dec.decode_many(blobs)
        side.synchronize()
        second, third = frames_of(second)[0], frames_of(third)[0]
    for a, b, c, w in zip(first, second, third, jpeg_cases.expected()[::9]):
        assert np.array_equal(a, w) and np.array_equal(b, w) and np.array_equal(c, w)
    got, refused = frames_of(dec.decode_many(blobs[3:4]))
    assert refused == {} and len(got) == 1 and np.array_equal(got[0], jpeg_cases.expected()[27])
    (flat, hw, offsets), refused = dec.decode_many([])
    assert flat.numel() == 0 and hw == [] and offsets == [] and refused == {}


def test_refused_files_are_reported_and_the_others_unaffected(dec):
    arr = jpeg_cases.pixels(40, 56, "ramp", 4)
    ok = [jpeg_cases.encode(jpeg_cases.pixels(h, w, "noise", h), s, 90) for h, w, s in ((40, 56, "420"), (33, 20, "422"), (8, 8, "gray"), (64, 64, "444"))]
    blobs = [ok[0], progressive(arr), ok[1], ok[0][:len(ok[0]) // 2], loud(np.full((16, 16, 3), 250, np.uint8)), ok[2], b"not a jpeg", ok[3]]
    got, refused = frames_of(dec.decode_many(blobs))
    assert refused == {1: UNSUPPORTED, 3: INVALID, 4: UNSUPPORTED, 6: INVALID}
    assert len(got) == 4
    for g, blob in zip(got, ok):
        assert np.array_equal(g, jpeg_cases.pil_rgb(blob))
    got, refused = frames_of(dec.decode_many([blobs[1], blobs[4]]))
    assert got == [] and refused == {0: UNSUPPORTED, 1: UNSUPPORTED}


# ----------------------------------------------------------------------------- the kernels over their whole input domain
DOMAIN_IMAGES = ((8, 8, 1, 1, 1), (8, 24, 3, 1, 1), (24, 17, 3, 2, 1), (16, 16, 3, 2, 2), (33, 65, 3, 2, 2))     # H, W, components, h, v


def domain_batch(table_value, seed):
    """Five parses in jpeg_ref's form whose coefficients no stream needs to give: per component the first blocks hold int16's
    extremes (all 32767, all -32768, their checkerboards by position, row and column, one extreme among zeros), the rest seeded
    values over all of int16, a third of them sparse; the tables hold `table_value` everywhere, or (None) a seeded choice among
    1, 255 and 65535 per entry."""
    rng, out = np.random.default_rng(seed), []
    k = np.arange(64)
    head = [np.full(64, 32767), np.full(64, -32768), np.where(k % 2, 32767, -32768), np.where((k // 8) % 2, -32768, 32767),
            np.where((k // 8 + k % 8) % 2, 32767, -32768)]
    for H, W, n, h, v in DOMAIN_IMAGES:
        mx, my = -(-W // (8 * h)), -(-H // (8 * v))
        coef = []
        for c in range(n):
            blocks = my * mx * (h * v if c == 0 else 1)
            a = rng.integers(-32768, 32768, (blocks, 64))
            a[rng.random((blocks, 64)) < 0.8 * (rng.random((blocks, 1)) < 1 / 3)] = 0
            if blocks > 2:
                for i, pattern in enumerate(head[c::n][:blocks - 2]):
                    a[i] = pattern
                a[-1] = 0
                a[-1, int(rng.integers(64))] = (32767, -32768)[c % 2]
            coef.append(a.astype(np.int16))
        quant = (np.full((n, 64), table_value) if table_value else rng.choice([1, 255, 65535], (n, 64))).astype(np.uint16)
        out.append({"height": H, "width": W, "components": n, "h": h, "v": v, "mcus_x": mx, "mcus_y": my, "restart": 0,
                    "coef": coef, "quant": quant})
    return out


@pytest.mark.parametrize("table_value", [1, 255, 65535, None])
def test_kernels_equal_the_header_over_the_whole_input_domain(cuda, ssd, table_value):
    """ssd_jpeg_decode by hand, as host_batch does, on tables and coefficients that come from no file: the frames equal
    jpeg_ref.pixels bit for bit where x = coefficient * q passes 2^31 and the sums of both passes wrap -- the uint32 arithmetic, the
    arithmetic shifts and the clamp of csrc/jpeg.hip against the header's definition, with PIL nowhere in it."""
    from importlib import import_module
    L, lib = import_module("ssd_amd._lib"), ssd.lib()
    batch = domain_batch(table_value, 11 if table_value is None else table_value)
    infos = (L.SsdJpegInfo * len(batch))()
    for info, p in zip(infos, batch):
        info.height, info.width, info.components, info.h, info.v = p["height"], p["width"], p["components"], p["h"], p["v"]
        info.mcus_x, info.mcus_y, info.restart_interval, info.reserved = p["mcus_x"], p["mcus_y"], 0, 0
        for c, a in enumerate(p["coef"]):
            info.blocks[c] = len(a)
        info.coef_count = 64 * sum(len(a) for a in p["coef"])
    table, totals = (L.SsdJpegImage * len(batch))(), (ctypes.c_int64 * 4)()
    assert lib.ssd_jpeg_plan(infos, len(batch), table, totals) == 0
    coef, quant = np.zeros(totals[0], np.int16), np.zeros(totals[1], np.uint16)
    for t, p in zip(table, batch):
        flat = np.concatenate([a.reshape(-1) for a in p["coef"]])
        coef[t.coef_offset:t.coef_offset + flat.size] = flat
        quant[t.quant_offset:t.quant_offset + p["quant"].size] = p["quant"].reshape(-1)
    want = [jpeg_ref.pixels(p) for p in batch]
    if table_value != 1:                                            # the batch does wrap: exact integers leave int32 in both passes
        x = np.abs(batch[4]["coef"][0].astype(np.int64) * batch[4]["quant"][0].astype(np.int64))
        assert x.max() >= 1 << 31 or x.reshape(-1, 8, 8).sum(1).max() * 8192 >= 1 << 31
    assert all(0 < np.count_nonzero((w > 0) & (w < 255)) < w.size for w in want[1:]), "clamped and unclamped samples (one block may clamp throughout)"
    arena = guarded.Arena(cuda, "cuda:0", "aligned")
    arena.add("table", np.frombuffer(bytes(table), np.uint8).copy(), np.uint8, 16, "input")
    arena.add("coef", coef.view(np.uint8), np.uint8, 16, "input")
    arena.add("quant", quant.view(np.uint8), np.uint8, 16, "input")
    arena.add("ws", (int(lib.ssd_jpeg_workspace_bytes(table, len(batch))),), np.uint8, 16, "workspace")
    arena.add("frames", (totals[3],), np.uint8, 16, "output", fill=0x3C)
    ssd._lib.check(lib.ssd_jpeg_decode(table, arena.ptr("table"), len(batch), arena.ptr("coef"), arena.ptr("quant"), arena.ptr("ws"),
                                       arena.ptr("frames"), None))
    cuda.cuda.synchronize()
    arena.check()
    out = arena.read("frames")
    for k, (t, w) in enumerate(zip(table, want)):
        got = out[t.frame_offset:t.frame_offset + w.size].reshape(w.shape)
        assert np.array_equal(got, w), "image %d: %d of %d bytes differ from the header's restatement" % (k, (got != w).sum(), w.size)


# ----------------------------------------------------------------------------- at and past the edge of the pinned rule
def edge_files():
    """[(name, blob, p)]: the loud, single-coefficient, colour-corner and upsampling files of tests/test_jpeg_loud_host.py."""
    return jpeg_loud.loud() + jpeg_loud.single() + jpeg_loud.corners() + jpeg_loud.upsampling()


def test_files_at_the_edge_of_the_rule_equal_pil_or_are_refused(dec):
    """One batch: every file the rule pins equals PIL bit for bit -- the IDCT's clamp up to v = -512 .. 511, the colour clamp at its
    corners, the upsampling's biases where they decide --, every other one is refused with SSD_ERR_UNSUPPORTED, in between them, and
    leaves its neighbours' frames alone."""
    files = edge_files()
    pinned = [jpeg_ref.pinned(p) for _n, _b, p in files]
    assert len(files) == 96 + 256 + 1 + 144 and sum(pinned) == 72 + 128 + 1 + 144
    got, refused = frames_of(dec.decode_many([blob for _n, blob, _p in files]))
    assert refused == {i: UNSUPPORTED for i, ok in enumerate(pinned) if not ok}
    kept = [f for f, ok in zip(files, pinned) if ok]
    assert len(got) == len(kept)
    bad = [name for (name, blob, _p), g in zip(kept, got) if not np.array_equal(g, jpeg_cases.pil_rgb(blob))]
    assert not bad, "%d frames differ from PIL, the first: %s" % (len(bad), bad[:5])


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def detector(cuda, ssd):
    """The model of tests/golden/tiny_mobilenet_128.npz (its seeded weights)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden as mg
    Wt, _img = mg.inputs()
    det = ssd.Detector(Wt, config=mg.TINY)
    yield det
    det.close()


def twelve_files():
    """12 JPEGs of three source sizes (three network shapes), samplings mixed, one progressive among them."""
    blobs = []
    for k in range(12):
        h, w = ((128, 128), (100, 151), (97, 203))[k % 3]
        arr = jpeg_cases.pixels(h, w, "noise" if k % 2 else "ramp", 50 + k)
        blobs.append(progressive(arr) if k == 7 else jpeg_cases.encode(arr, ("420", "444", "422", "gray")[k % 4], 90))
    return blobs


def test_detect_many_jpeg_equals_detect_many_on_pil_arrays(cuda, detector):
    blobs = twelve_files()
    arrays = [jpeg_cases.pil_rgb(b) for b in blobs]
    want = detector.detect_many(arrays, score_threshold=0.15, max_batch=4)
    got = detector.detect_many_jpeg(blobs, score_threshold=0.15, max_batch=4)
    assert sum(len(w[2]) for w in want) > 20
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    dev = "cuda:%d" % detector.device
    rec_want = detector.detect_many_records(arrays, detector.engine.new_records(12, dev).zero_(), max_batch=4)
    rec_got, shapes = detector.detect_many_records_jpeg(blobs, detector.engine.new_records(12, dev).zero_(), max_batch=4)
    assert cuda.equal(rec_want, rec_got) and shapes == [a.shape[:2] for a in arrays]


def test_refused_files_at_the_ends_and_across_group_boundaries(cuda, ssd, detector):
    """The twelve files with 0, 1, 4, 5 and 11 progressive as well (7 is): a refused file in the first row, in the last row and on both
    sides of the boundary between the decoder groups [0, 5) and [5, 10) (JPEG_GROUP = 5 on this instance: three groups), the
    accepted 128 x 128 files of the second group in non-consecutive rows, and the refused 100 x 151 files of the first group as
    ONE host batch into rows 1 and 4 (a fresh block and the indexed copy on the refused route too).  The rows equal pack_records of what detect_many's own
    batches produce for the PIL arrays -- mixed_batches' parts through Engine.detect_host_mixed, the call detect_many makes and
    nothing this route runs -- and detect_many_jpeg equals detect_many."""
    blobs = twelve_files()
    for k in (0, 1, 4, 5, 11):
        blobs[k] = progressive(jpeg_cases.pil_rgb(blobs[k]))
    arrays = [jpeg_cases.pil_rgb(b) for b in blobs]
    shapes = [a.shape[:2] for a in arrays]
    assert set(shapes) == {(128, 128), (100, 151), (97, 203)}
    parts = ssd.ssd.mixed_batches(detector.engine, shapes, 4)
    assert len({detector.engine.network_shape(*s) for s in shapes}) == 3          # (128 x 128, 128 x 256, 128 x 384: every part strides)
    assert all(p != list(range(p[0], p[0] + len(p))) for p in parts if len(p) > 1) and max(map(len, parts)) == 4
    want = np.zeros((12, detector.engine.record_words), np.int32)
    for part in parts:
        want[part] = ssd.ssd.pack_records(*detector.engine.detect_host_mixed([arrays[i] for i in part]))
    detector.JPEG_GROUP = 5
    try:
        assert detector._jpeg_groups(blobs) == [(0, 5), (5, 10), (10, 12)]
        rec = detector.engine.new_records(12, "cuda:%d" % detector.device).fill_(-1)
        got, got_shapes = detector.detect_many_records_jpeg(blobs, rec, max_batch=4)
        assert got is rec and cuda.equal(rec.cpu(), cuda.from_numpy(want)) and got_shapes == shapes
        many = detector.detect_many(arrays, score_threshold=0.15, max_batch=4)
        from_jpeg = detector.detect_many_jpeg(blobs, score_threshold=0.15, max_batch=4)
    finally:
        del detector.JPEG_GROUP
    assert sum(len(m[2]) for m in many) > 20
    for i, (m, j) in enumerate(zip(many, from_jpeg)):
        b, l, s, n = ssd.ssd.split_records(want[i:i + 1])
        for x, y, z in zip(m, j, ssd.ssd.score_filter(b[0], l[0], s[0], n[0], 0.15)):
            assert x.dtype == y.dtype == z.dtype and np.array_equal(x, y) and np.array_equal(x, z)


def test_coco_evaluate_from_jpeg_bytes_equals_the_default_route(cuda, ssd, detector, tmp_path):
    """coco_eval.evaluate(jpeg_device=0) on a folder of JPEGs (one progressive, one PNG under a .jpg name: both refused and read
    by the default reader): every statistic and the predictions file's bytes equal the default route's, alone and with rows_device."""
    cats = [{"id": i + 1 + (i > 10), "name": n} for i, n in enumerate(ssd.coco_eval.COCO_NAMES)]
    mapping = ssd.coco_eval.integer_to_coco_id(cats)
    from PIL import Image
    images, anns = [], []
    for k, blob in enumerate(twelve_files()):
        name = "%012d.jpg" % (k + 1)
        if k == 4:
            Image.fromarray(jpeg_cases.pil_rgb(blob)).save(str(tmp_path / name), "PNG")
        else:
            with open(tmp_path / name, "wb") as f:
                f.write(blob)
        im = np.asarray(Image.open(str(tmp_path / name)).convert("RGB"))
        images.append({"id": 1000 + k, "file_name": name, "height": im.shape[0], "width": im.shape[1]})
        for r in ssd.coco_eval.detection_records(detector, im, 1000 + k, mapping, score_threshold=0.3):
            x, y, w, h = r["bbox"]
            if w > 0 and h > 0:
                anns.append({"id": len(anns) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"],
                             "area": float(w * h), "iscrowd": 0})
    gt = {"images": images, "annotations": anns, "categories": cats}
    assert len(anns) > 10

    def run(name, **kw):
        path = str(tmp_path / name)
        stats = ssd.coco_eval.evaluate(detector, gt, str(tmp_path), predictions_json=path, max_batch=4, chunk=5, read_workers=4, **kw)
        return stats, open(path, "rb").read()
    base_stats, base_file = run("base.json")
    assert len(json.loads(base_file)) > 20
    for kw in ({"jpeg_device": 0}, {"jpeg_device": 0, "rows_device": 0}, {"jpeg_device": 0, "metric_device": 0}):
        stats, blob = run("jpeg.json", **kw)
        assert np.array_equal(np.asarray(stats), np.asarray(base_stats)), kw
        assert blob == base_file, kw
    with pytest.raises(ValueError):
        ssd.coco_eval.evaluate(detector, gt, str(tmp_path), predictions_json=None, jpeg_device=1)


def test_the_records_routes_refuse_alike(cuda, ssd, detector):
    """The refusals detect_many_records and detect_many_records_jpeg share, by type and text."""
    blobs = twelve_files()[:3]
    arrays = [jpeg_cases.pil_rgb(b) for b in blobs]
    dev = "cuda:%d" % detector.device
    routes = (("detect_many_records", lambda r: detector.detect_many_records(arrays, r)),
              ("detect_many_records_jpeg", lambda r: detector.detect_many_records_jpeg(blobs, r)))
    words = detector.engine.record_words
    for name, call in routes:
        detector.engine.set_precision("f16x3")
        try:
            with pytest.raises(ValueError) as e:
                call(detector.engine.new_records(3, dev))
        finally:
            detector.engine.set_precision("f32")
        assert str(e.value) == "%s runs in precision mode f32 only" % name
        for records in (cuda.zeros((3, words), dtype=cuda.int32), np.zeros((3, words), np.int32), None):
            with pytest.raises(ValueError) as e:
                call(records)
            assert str(e.value) == "records must be a tensor on cuda:%d" % detector.device
        for records in (detector.engine.new_records(4, dev), detector.engine.new_records(3, dev).float(),
                        detector.engine.new_records(6, dev)[::2]):
            with pytest.raises(ValueError) as e:
                call(records)
            assert str(e.value) == "records must be a contiguous int32 tensor [B, %d]" % words
    gt = {"images": [], "annotations": [], "categories": [{"id": i + 1, "name": n} for i, n in enumerate(ssd.coco_eval.COCO_NAMES)]}
    for bad in ({"detector": detector, "jpeg_device": detector.device + 1}, {"detector": lambda im, score_threshold: None, "jpeg_device": 0}):
        with pytest.raises(ValueError) as e:
            ssd.coco_eval.evaluate(bad["detector"], gt, "", predictions_json=None, jpeg_device=bad["jpeg_device"])
        assert str(e.value) == "jpeg_device must be the GPU of a Detector: the frames are detected where they are decoded"


def test_routes_with_refused_loud_files_equal_the_pil_array_routes(cuda, dec, detector):
    """detect_many_jpeg and detect_many_records_jpeg on the twelve files with two of them (a 128 x 128 and a 100 x 151 one) under
    constant tables past the rule: the parser takes them, ssd_jpeg_entropy refuses them, the caller's reader decodes them, and the
    results equal the routes on PIL's arrays."""
    blobs = twelve_files()
    for k, value in ((3, 255), (4, 200)):
        tables = 1 if k % 4 == 3 else 2                              # (twelve_files' sampling order: every fourth is grayscale)
        blobs[k] = jpeg_loud.constant_tables(blobs[k], [value] * tables)
    assert all(dec.read_info(blobs[k])[0] == 0 for k in (3, 4))
    assert frames_of(dec.decode_many([blobs[3], blobs[4]])) == ([], {0: UNSUPPORTED, 1: UNSUPPORTED})
    arrays = [jpeg_cases.pil_rgb(b) for b in blobs]
    want = detector.detect_many(arrays, score_threshold=0.15, max_batch=4)
    got = detector.detect_many_jpeg(blobs, score_threshold=0.15, max_batch=4)
    assert sum(len(w[2]) for w in want) > 20
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    dev = "cuda:%d" % detector.device
    rec_want = detector.detect_many_records(arrays, detector.engine.new_records(12, dev).zero_(), max_batch=4)
    rec_got, shapes = detector.detect_many_records_jpeg(blobs, detector.engine.new_records(12, dev).zero_(), max_batch=4)
    assert cuda.equal(rec_want, rec_got) and shapes == [a.shape[:2] for a in arrays]
