"""-m gpu: the JPEG encoder (include/ssd_hip.h, block "the JPEG encoder"; csrc/jpeg_enc.hip, csrc/jpeg_emit.cpp, jpeg.py) against
the encoder the reference uses, PIL's Image.save(format="jpeg"): coefficients equal the numpy restatement bit for bit and files
equal PIL's byte for byte -- the shared case list as one batch and reversed, images past one grid pass of either launch, the call
between guard words at 16-byte-not-32-byte addresses, a side stream, the edge batch sizes, the round trip through JpegDecoder, and
the route built on it: create_tfrecords --jpeg_device, whose shards equal the default route's and feed TrainPipeline."""
import ctypes
import os
from importlib import import_module

import numpy as np
import pytest

from tests.helpers import data_prep_cases, guarded, jpeg_cases, jpeg_enc_cases, jpeg_enc_ref

pytestmark = pytest.mark.gpu
GRID_CAP = 1024                     # SSD_COCO_GRID_CAP: groups of a launch; 256 units (launch 1) / 32 blocks (launch 2) per group and pass
CODE = jpeg_enc_cases.CODE


@pytest.fixture(scope="module")
def enc(cuda, ssd):
    return ssd.JpegEncoder(0)


@pytest.fixture(scope="module")
def L(ssd):
    return import_module("ssd_amd._lib")


def plan(ssd, L, frames, qualities, samplings):
    rows = np.asarray([(f.shape[0], f.shape[1], CODE[s], q) for f, q, s in zip(frames, qualities, samplings)], np.int32).reshape(-1, 4)
    table, totals = (L.SsdJpegEncodeImage * len(frames))(), (ctypes.c_int64 * 4)()
    assert ssd.lib().ssd_jpeg_encode_plan(rows.ctypes.data, len(frames), table, totals) == 0
    return table, list(totals)


def device_coefficients(cuda, ssd, L, frames, qualities, samplings):
    """ssd_jpeg_encode by hand on one batch -> (table, int16 coefficients of the whole batch)."""
    lib = ssd.lib()
    table, totals = plan(ssd, L, frames, qualities, samplings)
    flat = np.zeros(totals[2], np.uint8)
    for t, f in zip(table, frames):
        flat[t.frame_offset:t.frame_offset + f.size] = f.reshape(-1)
    dev_frames = cuda.from_numpy(flat).cuda()
    dev_table = cuda.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    ws = cuda.empty(int(lib.ssd_jpeg_encode_workspace_bytes(table, len(frames))), dtype=cuda.uint8, device="cuda:0")
    coef = cuda.full((int(totals[0]),), 0x5A5A, dtype=cuda.int16, device="cuda:0")
    ssd._lib.check(lib.ssd_jpeg_encode(table, dev_table.data_ptr(), len(frames), dev_frames.data_ptr(), ws.data_ptr(), coef.data_ptr(), None))
    cuda.cuda.synchronize()
    return table, coef.cpu().numpy()


def test_whole_case_list_as_one_batch_and_reversed(cuda, ssd, L, enc):
    """The 216 frames -- every size, content, quality and sampling -- as ONE batch, forwards and reversed."""
    cases = jpeg_enc_cases.cases()
    for order in (cases, cases[::-1]):
        frames, qualities, samplings = [c[1] for c in order], [c[2] for c in order], [c[3] for c in order]
        table, coef = device_coefficients(cuda, ssd, L, frames, qualities, samplings)
        bad = [c[0] for c, t in zip(order, table)
               if not np.array_equal(coef[t.coef_offset:t.coef_offset + 64 * ((t.h * t.v + 2) * t.mcus_x * t.mcus_y)],
                                     jpeg_enc_ref.flat(c[1], c[2], c[3]))]
        assert not bad, "%d coefficient runs differ from the restatement, the first: %s" % (len(bad), bad[:5])
        got = enc.encode_many([cuda.from_numpy(np.array(f)).cuda() for f in frames], qualities, samplings)
        bad = [c[0] for c, g in zip(order, got) if g != c[4]]
        assert len(got) == 216 and not bad, "%d files differ from PIL's, the first: %s" % (len(bad), bad[:5])


def big(h, w, seed):
    """uint8 [h, w, 3]: two ramps and a little noise, made with integer arithmetic (cheap at megapixels)."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(h, dtype=np.int32)[:, None, None], np.arange(w, dtype=np.int32)[None, :, None]
    return ((y * 3 + x * 5) // 8 + np.arange(3, dtype=np.int32) * 70 + rng.integers(0, 24, (h, w, 3), dtype=np.int32)).astype(np.uint8)


def test_past_one_grid_pass_of_both_launches(cuda, ssd, enc):
    """Five 4:2:0 frames of 7200 blocks (36 000 > 1024 x 32: launch 2's stride loop runs twice over a batch, one frame with dummy
    blocks right and below), and for launch 1 the smallest images that ALONE exceed its pass of 1024 x 256 units (8 mcus_y mcus_x
    > 262 144): 1456 x 1448 at 4:4:4 (263 536 units, 98 826 blocks) and 2890 x 2900 at 4:2:0 (263 536 units, 197 652 blocks)."""
    a, b = jpeg_cases.pixels(480, 640, "ramp", 1), jpeg_cases.pixels(420, 630, "noise", 2)
    batch = [a, b, a, b, a]
    lib = ssd.lib()
    assert (53 * 79, 27 * 40 * 4) == ((420 + 7) // 8 * ((630 + 7) // 8), 4320)         # b: 133 dummy blocks
    assert sum(6 * -(-f.shape[0] // 16) * -(-f.shape[1] // 16) for f in batch) > GRID_CAP * 32
    got = enc.encode_many([cuda.from_numpy(f).cuda() for f in batch], 75, "420")
    assert got == [jpeg_cases.encode(f, "420", 75) for f in batch]
    for (h, w), sampling, mcu in (((1456, 1448), "444", 8), ((2890, 2900), "420", 16)):
        assert 8 * -(-h // mcu) * -(-w // mcu) > GRID_CAP * 256 >= 8 * (-(-h // mcu) - 1) * -(-w // mcu)
        frame = big(h, w, h)
        got = enc.encode_many([cuda.from_numpy(frame).cuda(), cuda.from_numpy(a).cuda()], 75, sampling)
        assert len(got[0]) <= lib.ssd_jpeg_emit_bound(h, w, CODE[sampling])
        assert got[0] == jpeg_cases.encode(frame, sampling, 75), (h, w, sampling)
        assert got[1] == jpeg_cases.encode(a, sampling, 75)


@pytest.mark.parametrize("layout", ["skewed", "aligned"])
def test_between_guard_words_every_coefficient_written_once(cuda, ssd, L, layout):
    """Table, frames, workspace and coefficients in ONE arena between guard words (skewed: the 16-byte bases 16 and not 32 bytes
    aligned, the frames at 4 mod 16), the images' coefficient runs and planes spread apart by hand: every coefficient is written
    whatever it held before, the values between two images' runs keep what they held, no guard and no input changes -- the planes
    are written inside the workspace only."""
    lib = ssd.lib()
    picks = jpeg_enc_cases.cases()[::5]                                      # every size, content, quality and sampling
    for extra in ("420", "444"):
        frames = [c[1] for c in picks] + [jpeg_cases.pixels(150, 211, "ramp", 9)]
        qualities, samplings = [c[2] for c in picks] + [75], [c[3] for c in picks] + [extra]
        table, totals = plan(ssd, L, frames, qualities, samplings)
        flat = np.zeros(totals[2], np.uint8)
        for k, (t, f) in enumerate(zip(table, frames)):
            flat[t.frame_offset:t.frame_offset + f.size] = f.reshape(-1)
            t.coef_offset += 8 * k * (k + 1)                # gaps of 16 k int16 between the runs
            t.plane_offset += 16 * k
        n_coef = table[-1].coef_offset + 64 * (totals[3] - table[-1].block_begin)
        ws_bytes = int(lib.ssd_jpeg_encode_workspace_bytes(table, len(frames)))
        assert ws_bytes == totals[1] + 16 * (len(frames) - 1)
        inside = np.zeros(n_coef, bool)
        want = np.zeros(n_coef, np.int16)
        for t, f, q, smp in zip(table, frames, qualities, samplings):
            ref = jpeg_enc_ref.flat(f, q, smp)
            inside[t.coef_offset:t.coef_offset + ref.size] = True
            want[t.coef_offset:t.coef_offset + ref.size] = ref
        assert (~inside).sum() == 16 * sum(range(len(frames)))
        for fill in (0x3C3C, -0x3C3D):
            arena = guarded.Arena(cuda, "cuda:0", layout)
            arena.add("table", np.frombuffer(bytes(table), np.uint8).copy(), np.uint8, 16, "input")
            arena.add("frames", flat, np.uint8, 4, "input")
            arena.add("ws", (ws_bytes,), np.uint8, 16, "workspace")
            arena.add("coef", (2 * n_coef,), np.uint8, 16, "output", fill=np.full(n_coef, fill, np.int16).view(np.uint8))
            if layout == "skewed":
                assert all(arena.ptr(n) % 32 == 16 for n in ("table", "ws", "coef")) and arena.ptr("frames") % 16 != 0
            ssd._lib.check(lib.ssd_jpeg_encode(table, arena.ptr("table"), len(frames), arena.ptr("frames"), arena.ptr("ws"),
                                               arena.ptr("coef"), None))
            cuda.cuda.synchronize()
            arena.check()
            out = arena.read("coef").view(np.int16)
            assert np.all(out[~inside] == fill), "a value between two images' coefficients was written"
            assert np.array_equal(out[inside], want[inside]), "fill %x" % fill


def test_side_stream_second_call_and_edge_batches(cuda, enc):
    cases = [c for c in jpeg_enc_cases.cases() if c[2] == 75 and c[3] == "420"][::3]
    frames = [cuda.from_numpy(np.array(c[1])).cuda() for c in cases]
    want = [c[4] for c in cases]
    assert enc.encode_many(frames) == want                                  # the defaults: quality 75, 4:2:0
    side = cuda.cuda.Stream()
    with cuda.cuda.stream(side):
        first = enc.begin(frames)
        second = enc.begin(frames)                                          # both pinned buffers in flight
        with pytest.raises(RuntimeError):
            enc.begin(frames)
        assert enc.finish(first) == want and enc.finish(second) == want
    assert enc.encode_many(frames[3:4]) == want[3:4]                        # B = 1
    assert enc.encode_many([]) == []                                        # B = 0
    assert enc.encode_many([np.array(c[1]) for c in cases]) == want         # host arrays: one pinned upload
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:
        assert enc.encode_many(frames, pool=pool) == want
    for bad in ("422", "gray", 411):
        with pytest.raises(ValueError):
            enc.encode_many(frames, sampling=bad)
    for bad in (0, 101, 75.0, [75]):
        with pytest.raises(ValueError):
            enc.encode_many(frames, quality=bad)
    with pytest.raises(ValueError):
        enc.encode_many([frames[0].float()])


def test_round_trip_through_the_decoder_equals_pil(cuda, ssd, enc):
    """JpegDecoder.decode_many(JpegEncoder.encode_many(x)) == PIL.open(PIL-encoded x).convert("RGB"), and the decoder's own tuple
    goes back into the encoder where it lies."""
    dec = ssd.JpegDecoder(0)
    cases = [c for c in jpeg_enc_cases.cases() if c[2] == 75][::2]
    for sampling in ("420", "444"):
        part = [c for c in cases if c[3] == sampling]
        blobs = enc.encode_many([cuda.from_numpy(np.array(c[1])).cuda() for c in part], 75, sampling)
        (flat, hw, offsets), refused = dec.decode_many(blobs)
        assert refused == {} and hw == [c[1].shape[:2] for c in part]
        host = flat.cpu().numpy()
        for c, (h, w), o in zip(part, hw, offsets):
            assert np.array_equal(host[o:o + 3 * h * w].reshape(h, w, 3), jpeg_cases.pil_rgb(c[4])), c[0]
        again = enc.encode_many((flat, hw, offsets), 75, sampling)
        assert again == [jpeg_cases.encode(jpeg_cases.pil_rgb(c[4]), sampling, 75) for c in part]
    assert ssd.Detector.jpeg_encoder is not None and isinstance(ssd.jpeg.JpegEncoder(0), ssd.JpegEncoder)


def test_create_tfrecords_on_the_gpu_equals_the_default_route_and_feeds_the_pipeline(cuda, ssd, tmp_path):
    create = import_module("ssd_amd.create_tfrecords")
    root = str(tmp_path / "prep")
    os.mkdir(root)
    entries = data_prep_cases.make_folder(root)
    # a grayscale PNG under a .jpg name: the decoder refuses it, PIL reads it, the encoder takes the staged frame
    from PIL import Image
    import json
    arr = jpeg_cases.pixels(31, 45, "ramp", 77)[:, :, 1]
    Image.fromarray(arr).save(os.path.join(root, "images", "h_gray_png.jpg"), format="PNG")
    with open(os.path.join(root, "annotations", "h_gray_png.json"), "w") as f:
        json.dump({"filename": "h_gray_png.jpg", "size": {"depth": 3, "width": 45, "height": 31},
                   "object": [{"bndbox": {"ymin": 2, "ymax": 20, "xmax": 40, "xmin": 3}, "name": "cat"}]}, f)

    def run(out, **kw):
        return create.create(os.path.join(root, "images"), os.path.join(root, "annotations"), out, os.path.join(root, "labels.txt"),
                             num_shards=3, seed=5, **kw)
    host, gpu = str(tmp_path / "host"), str(tmp_path / "gpu")
    want = run(host)
    got = run(gpu, jpeg_device=0)
    assert got == want == {"examples": 8, "written": 6, "skipped": 2, "shards": 2, "shard_size": 3}
    assert sorted(os.listdir(gpu)) == sorted(os.listdir(host)) == ["shard-0000.tfrecords", "shard-0001.tfrecords"]
    for name in os.listdir(host):
        assert open(os.path.join(gpu, name), "rb").read() == open(os.path.join(host, name), "rb").read(), name
    stored = [ssd.tfrecords.parse_example(r)["image"][0] for n in sorted(os.listdir(gpu)) for r in ssd.tfrecords.read_records(os.path.join(gpu, n))]
    assert sum(b == data_prep_cases.stored_image(e) for b in stored for e in entries.values() if e["kind"] == "gray") == 2
    pipe = ssd.TrainPipeline(gpu, {"batch_size": 4, "image_height": 128, "image_width": 128}, seed=3, read_workers=2)
    images, gt = next(pipe)
    assert tuple(images.shape) == (4, 128, 128, 3) and images.is_cuda and set(gt) == {"boxes", "labels", "num_boxes"}
    assert int(gt["num_boxes"].sum()) > 0 and float(images.max()) <= 1 and float(images.min()) >= 0
