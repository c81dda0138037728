"""The TRAIN input pipeline without a GPU: the float32 restatement of ssd_augment (tests/helpers/augment_ref.py) on
hand-worked frames, its Philox against rocRAND's, the crop sampler's properties, the box steps, the record stream
(shards, shuffle buffer, epochs, batching) on a stub decoder, and the C entry point's refusals."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import augment_ref, example_protos

f32 = np.float32
U = f32(1.0 / 255.0)


def _params(ssd, H, W, crop=None, flags=0, offsets=(0, 0, 0), key=0):
    from ssd_amd import augment
    p = np.zeros((), augment.PARAMS_DTYPE)
    p["height"], p["width"] = H, W
    p["crop_y"], p["crop_x"], p["crop_h"], p["crop_w"] = crop or (0, 0, H, W)
    p["flags"], p["color_offset"], p["philox_key"] = flags, offsets, key
    p["scale_min"], p["scale_range"] = f32(0.85), f32(1.15) - f32(0.85)
    return p[()]


FRAME23 = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 10


def test_ref_resizes_a_2x3_frame_up_and_down(ssd):
    up = augment_ref.augment(FRAME23, _params(ssd, 2, 3), 4, 6)
    # rows floor(y * 0.5) = 0 0 1 1; columns floor(x * 0.5) = 0 0 1 1 2 2
    want = FRAME23[[0, 0, 1, 1]][:, [0, 0, 1, 1, 2, 2]].astype(np.float32) * U
    assert np.array_equal(up, want)
    down = augment_ref.augment(FRAME23, _params(ssd, 2, 3), 1, 2)
    # rows floor(y * 2) = 0; columns floor(x * 1.5) = 0 1
    assert np.array_equal(down, FRAME23[[0]][:, [0, 1]].astype(np.float32) * U)
    odd = augment_ref.augment(FRAME23, _params(ssd, 2, 3), 3, 4)
    # rows floor(y * 2/3) = 0 0 1; columns floor(x * 0.75) = 0 0 1 2
    assert np.array_equal(odd, FRAME23[[0, 0, 1]][:, [0, 0, 1, 2]].astype(np.float32) * U)


@pytest.mark.parametrize("crop,rows,cols", [
    ((0, 0, 2, 3), [0, 0, 1, 1], [0, 0, 1, 1, 2, 2]),            # top-left corner
    ((3, 4, 2, 3), [3, 3, 4, 4], [4, 4, 5, 5, 6, 6]),            # bottom-right corner
    ((0, 2, 5, 2), [0, 1, 2, 3], [2, 2, 2, 3, 3, 3]),            # top and bottom edges
    ((2, 0, 1, 7), [2, 2, 2, 2], [0, 1, 2, 3, 4, 5]),            # left and right edges, one row
])
def test_ref_crop_window_at_every_edge(ssd, crop, rows, cols):
    frame = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    got = augment_ref.augment(frame, _params(ssd, 5, 7, crop), 4, 6)
    assert np.array_equal(got, frame[rows][:, cols].astype(np.float32) * U)


def test_ref_colour_clips_at_0_and_1(ssd):
    frame = np.array([[[250, 3, 128]]], np.uint8)
    got = augment_ref.augment(frame, _params(ssd, 1, 1, flags=1, offsets=(0.1, -0.1, 0.0)), 1, 1)
    assert got[0, 0, 0] == f32(1) and got[0, 0, 1] == f32(0)
    assert got[0, 0, 2] == f32(128) * U
    got = augment_ref.augment(frame, _params(ssd, 1, 1, flags=1, offsets=(0.01, 0.02, -0.25)), 1, 1)
    assert got[0, 0, 0] == f32(250) * U + f32(0.01) and got[0, 0, 1] == f32(3) * U + f32(0.02)
    assert got[0, 0, 2] == f32(128) * U - f32(0.25)


def test_ref_grayscale(ssd):
    frame = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]]], np.uint8)
    got = augment_ref.augment(frame, _params(ssd, 1, 4, flags=2), 1, 4)
    want = [f32(0.2989), f32(0.5870), f32(0.1140), (f32(0.2989) + f32(0.5870)) + f32(0.1140)]
    for i, w in enumerate(want):
        assert np.all(got[0, i] == w), (i, got[0, i], w)


def test_ref_flip_and_channels_first(ssd):
    plain = augment_ref.augment(FRAME23, _params(ssd, 2, 3), 4, 6)
    flipped = augment_ref.augment(FRAME23, _params(ssd, 2, 3, flags=8), 4, 6)
    assert np.array_equal(flipped, plain[:, ::-1])
    assert np.array_equal(augment_ref.augment(FRAME23, _params(ssd, 2, 3, flags=8), 4, 6, channels_first=True),
                          flipped.transpose(2, 0, 1))


def test_ref_pixel_scale_uses_pre_flip_coordinates(ssd):
    frame = np.full((2, 3, 3), 128, np.uint8)
    a = augment_ref.augment(frame, _params(ssd, 2, 3, flags=4, key=0x0123456789ABCDEF), 2, 4)
    b = augment_ref.augment(frame, _params(ssd, 2, 3, flags=4 | 8, key=0x0123456789ABCDEF), 2, 4)
    assert np.array_equal(b, a[:, ::-1])
    words = augment_ref.philox4x32_10([1 * 4 + 2], 0x0123456789ABCDEF)[0]
    f = augment_ref.uint_to_unit(words[:3]) * (f32(1.15) - f32(0.85)) + f32(0.85)
    assert np.array_equal(a[1, 2], np.clip((f32(128) * U) * f, f32(0), f32(1)))


def test_philox_known_answers():
    """Random123's known answers for Philox4x32-10 (counter 0, key 0 and counter all ones, key all ones do not fit the
    (c, 0, 0, 0) form; counter 0 / key 0 does)."""
    assert [hex(w) for w in augment_ref.philox4x32_10([0], 0)[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    u = augment_ref.uint_to_unit(np.array([0, 0xFFFFFFFF, 0x00400000], np.uint32))
    assert u[0] == 0 and u[1] == f32(1) - f32(2.0 ** -23) and u[2] == f32(0.5)


def test_philox_matches_rocrand(tmp_path):
    """The helper's Philox4x32-10 against rocRAND's header-only philox4x32_10_engine, evaluated on the host in a small
    program built here (seed = key, the counter reached by skipping 4 * c numbers)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hdr = "/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"
    if not (shutil.which(hipcc) or os.path.exists(hipcc)) or not os.path.exists(hdr):
        pytest.skip("rocRAND's headers or hipcc are not installed")
    src = tmp_path / "philox.cpp"
    src.write_text("""
#include <rocrand/rocrand_philox4x32_10.h>
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    const unsigned long long key = strtoull(argv[1], 0, 0);
    for (int i = 2; i < argc; ++i) {
        rocrand_device::philox4x32_10_engine e(key, 0, 4ull * strtoull(argv[i], 0, 0));
        const uint4 r = e.next4();
        printf("%u %u %u %u\\n", r.x, r.y, r.z, r.w);
    }
    return 0;
}
""")
    exe = tmp_path / "philox"
    subprocess.check_call([hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O1", str(src), "-o", str(exe)])
    rng = np.random.default_rng(5)
    for key in (0, 0xDEADBEEFDEADBEEF, int(rng.integers(0, 2 ** 63)) * 2 + 1):
        ctrs = [0, 1, 2, 639, 640 * 640 - 1, 0xFFFFFFFF] + [int(c) for c in rng.integers(0, 2 ** 32, 10)]
        out = subprocess.check_output([str(exe), str(key)] + [str(c) for c in ctrs], text=True)
        want = np.array([[int(w) for w in line.split()] for line in out.splitlines()], np.uint64)
        assert np.array_equal(augment_ref.philox4x32_10(ctrs, key).astype(np.uint64), want), key


# ----------------------------------------------------------------------------- the crop sampler
def _rects(boxes, H, W):
    return [(int(b[0] * f32(H)), int(b[1] * f32(W)), int(b[2] * f32(H)), int(b[3] * f32(W))) for b in boxes]


def test_crop_sampler_properties():
    from ssd_amd import augment
    rng = np.random.default_rng(7)
    fallbacks = 0
    for t in range(400):
        # near-square frames: a window of area >= 0.67 and aspect in [0.8, 1.2] exists (a 20 x 900 frame has none)
        H = int(rng.integers(20, 900))
        W = max(20, int(round(H * rng.uniform(0.9, 1.1))))
        n = int(rng.integers(0, 5))
        c = rng.random((n, 2)) * 0.8
        s = rng.random((n, 2)) * 0.5 + 0.02
        boxes = np.clip(np.concatenate([c, c + s], 1)[:, [0, 1, 2, 3]], 0, 1).astype(np.float32)
        y, x, h, w = augment.sample_distorted_bounding_box(rng, H, W, boxes, 0.5, (0.8, 1.2), (0.67, 0.97))
        assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= H and x + w <= W
        if (y, x, h, w) == (0, 0, H, W):
            fallbacks += 1
            continue
        area = f32(h * w)
        assert f32(0.67) * f32(W) * f32(H) <= area <= f32(0.97) * f32(W) * f32(H)
        # the aspect ratio drawn lies in [0.8, 1.2]; w = lrint(h * ar) allows half a pixel either side
        assert 0.8 * h - 0.5 - 1e-3 <= w <= 1.2 * h + 0.5 + 1e-3
        rects = _rects(boxes, H, W) or [(0, 0, H, W)]
        covered = [max(0, min(y + h, r[2]) - max(y, r[0])) * max(0, min(x + w, r[3]) - max(x, r[1])) / ((r[2] - r[0]) * (r[3] - r[1]))
                   for r in rects if (r[2] - r[0]) > 0 and (r[3] - r[1]) > 0]
        assert max(covered) >= 0.5 - 1e-6
    assert fallbacks < 40


def test_crop_sampler_without_boxes_uses_area_and_aspect_only():
    from ssd_amd import augment
    rng = np.random.default_rng(3)
    for _ in range(200):
        y, x, h, w = augment.sample_distorted_bounding_box(rng, 480, 640, np.zeros((0, 4), np.float32), 0.5, (0.8, 1.2), (0.67, 0.97))
        assert (y, x, h, w) != (0, 0, 480, 640)
        assert f32(0.67) * f32(640) * f32(480) <= f32(h * w) <= f32(0.97) * f32(640) * f32(480)
        assert y + h <= 480 and x + w <= 640


def test_crop_sampler_falls_back_to_the_whole_image():
    from ssd_amd import augment
    # a box of no pixel area can never be covered: every attempt fails
    boxes = np.array([[0.5, 0.5, 0.5001, 0.9]], np.float32)
    assert augment.sample_distorted_bounding_box(np.random.default_rng(0), 100, 100, boxes, 0.5, (0.8, 1.2), (0.67, 0.97)) == (0, 0, 100, 100)


def test_sampler_same_seed_same_draws():
    from ssd_amd import augment
    boxes = np.array([[0.1, 0.1, 0.6, 0.5], [0.4, 0.5, 0.9, 0.95]], np.float32)

    def run(seed):
        rng = np.random.default_rng(seed)
        return [augment.sample_augmentation(rng, 333, 500, boxes, [1, 2]) for _ in range(50)]
    a, b, c = run(11), run(11), run(12)
    for (pa, ba, la), (pb, bb, lb) in zip(a, b):
        assert pa.tobytes() == pb.tobytes() and np.array_equal(ba, bb) and np.array_equal(la, lb)
    assert any(pa.tobytes() != pc.tobytes() for (pa, _, _), (pc, _, _) in zip(a, c))


def test_sampler_flag_frequencies_and_params():
    from ssd_amd import augment
    rng = np.random.default_rng(0)
    n = 4000
    rows = [augment.sample_augmentation(rng, 200, 300, np.zeros((0, 4)), [])[0] for _ in range(n)]
    fl = np.array([int(r["flags"]) for r in rows])
    cropped = np.array([(int(r["crop_h"]), int(r["crop_w"])) != (200, 300) for r in rows])
    assert abs(cropped.mean() - 0.95) < 0.02
    assert abs((fl & 8 > 0).mean() - 0.5) < 0.04 and abs((fl & 1 > 0).mean() - 0.05) < 0.015
    assert abs((fl & 4 > 0).mean() - 0.05) < 0.015 and (fl & 2 > 0).mean() < 0.03
    for r in rows:
        assert r["scale_min"] == f32(0.85) and r["scale_range"] == f32(1.15) - f32(0.85)
        if r["flags"] & 1:
            assert np.all(np.abs(r["color_offset"]) < 32 / 255 + 0.1 * 1.772 + 1e-6)


# ----------------------------------------------------------------------------- box steps
def test_prune_non_overlapping_exactly_at_ioa_0_3():
    from ssd_amd import augment
    window = np.array([0.0, 0.0, 0.5, 1.0], np.float32)
    # box of height 0.4 (area 0.4 * 0.5): 0.12 of it inside the window -> IOA 0.3 up to the epsilon; nudged both ways
    boxes = np.array([[0.38, 0.0, 0.78, 0.5], [0.3805, 0.0, 0.7805, 0.5], [0.3795, 0.0, 0.7795, 0.5]], np.float32)
    ioa = augment.ioa(window[None, :], boxes)[0]
    kept, keep = augment.prune_non_overlapping_boxes(boxes, window, 0.3)
    assert list(keep) == [i for i in range(3) if ioa[i] >= f32(0.3)]
    assert 2 in keep and 1 not in keep
    # IOA exactly 0.3 in float32 is kept (>=): a box whose intersection / (area + eps) rounds to f32(0.3)
    b = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    w = np.array([0.0, 0.0, 1.0, 0.3], np.float32)
    assert augment.ioa(w[None, :], b)[0, 0] == f32(0.3) and list(augment.prune_non_overlapping_boxes(b, w, 0.3)[1]) == [0]


def test_prune_completely_outside_window():
    from ssd_amd import augment
    window = np.array([0.2, 0.2, 0.6, 0.6], np.float32)
    boxes = np.array([[0.6, 0.3, 0.9, 0.5],      # starts at the window's bottom: outside
                      [0.0, 0.0, 0.2, 0.5],      # ends at its top: outside
                      [0.1, 0.1, 0.3, 0.3],      # overlaps a corner
                      [0.7, 0.7, 0.9, 0.9]], np.float32)
    kept, idx = augment.prune_completely_outside_window(boxes, window)
    assert list(idx) == [2] and np.array_equal(kept, boxes[[2]])


def test_change_coordinate_frame_clips():
    from ssd_amd import augment
    window = np.array([0.25, 0.5, 0.75, 1.0], np.float32)
    boxes = np.array([[0.0, 0.6, 0.5, 0.8], [0.3, 0.75, 1.0, 1.0]], np.float32)
    got = augment.change_coordinate_frame(boxes, window)
    want = np.array([[0.0, (f32(0.6) - f32(0.5)) / f32(0.5), 0.5, (f32(0.8) - f32(0.5)) / f32(0.5)],
                     [(f32(0.3) - f32(0.25)) / f32(0.5), 0.5, 1.0, 1.0]], np.float32)
    assert np.array_equal(got, want)


def test_jitter_clips_and_flip():
    from ssd_amd import augment
    boxes = np.array([[0.0, 0.1, 0.5, 0.995], [0.2, 0.2, 0.4, 0.6]], np.float32)
    rand = np.array([[-0.01, 0.01, 0.01, 0.01], [0.005, -0.005, 0.0, 0.01]], np.float32)
    got = augment.jitter_boxes(boxes, rand)
    assert got[0, 0] == 0 and got[0, 3] == 1.0                  # clipped at both ends
    assert got[0, 1] == f32(0.1) + f32(f32(0.995) - f32(0.1)) * f32(0.01)
    assert got[1, 0] == f32(0.2) + f32(f32(0.4) - f32(0.2)) * f32(0.005)
    fl = augment.flip_boxes(boxes)
    assert np.array_equal(fl, np.array([[0.0, f32(1) - f32(0.995), 0.5, f32(1) - f32(0.1)],
                                        [0.2, f32(1) - f32(0.6), 0.4, f32(1) - f32(0.2)]], np.float32))


def test_labels_follow_their_boxes():
    """Every kept box comes back with its own label, whatever was pruned: labels encode their box."""
    from ssd_amd import augment
    rng = np.random.default_rng(9)
    for _ in range(300):
        n = int(rng.integers(1, 8))
        c = rng.random((n, 2)) * 0.85
        boxes = np.concatenate([c, c + 0.03 + rng.random((n, 2)) * 0.12], 1).astype(np.float32)
        labels = np.arange(n, dtype=np.int32) + 10
        p, bx, lb = augment.sample_augmentation(rng, 400, 500, boxes, labels, {"jitter_ratio": 0.0})
        y, x, h, w = (int(p[k]) for k in ("crop_y", "crop_x", "crop_h", "crop_w"))
        window = np.array([f32(y) / f32(400), f32(x) / f32(500), f32(y + h) / f32(400), f32(x + w) / f32(500)], np.float32)
        src = boxes[lb - 10]
        want = augment.change_coordinate_frame(src, window) if (h, w) != (400, 500) or len(lb) == n else src
        if p["flags"] & 8:
            want = augment.flip_boxes(want)
        assert len(set(lb.tolist())) == len(lb) and np.array_equal(bx, want)


def test_color_offsets_in_the_reference_order():
    from ssd_amd import augment
    o = augment.color_offsets(0.1, -0.05, 0.07)
    assert o[0] == f32(1.402) * f32(0.07) + f32(0.1)
    assert o[1] == (f32(-0.344136) * f32(-0.05) - f32(0.714136) * f32(0.07)) + f32(0.1)
    assert o[2] == f32(1.772) * f32(-0.05) + f32(0.1)


# ----------------------------------------------------------------------------- the record stream
def test_shuffle_buffer_semantics():
    from ssd_amd import augment
    out = list(augment.shuffle_buffer(range(50), 4, np.random.default_rng(0)))
    assert sorted(out) == list(range(50))
    # the k-th output was in the buffer: it is one of the first k + 4 inputs
    assert all(v < k + 4 for k, v in enumerate(out))
    assert out != list(range(50))
    assert list(augment.shuffle_buffer(range(5), 1, np.random.default_rng(0))) == list(range(5))


def _write_shards(tmp_path, counts):
    from ssd_amd import tfrecords
    k = 0
    for s, n in enumerate(counts):
        recs = []
        for _ in range(n):
            # the stub "JPEG" is the record's id; boxes differ per record
            recs.append(example_protos.example_bytes(b"id%05d" % k, [[0.1, 0.1, 0.5 + 0.001 * k, 0.6]], [k % 7]))
            k += 1
        tfrecords.write_records(str(tmp_path / ("train-%02d.tfrecords" % s)), recs)
    return k


def _stub_decode(jpeg):
    k = int(jpeg[2:])
    return np.full((40 + k % 9, 50 + k % 5, 3), k % 256, np.uint8)


def test_records_once_per_epoch_and_remainder_dropped(tmp_path):
    from ssd_amd import augment
    total = _write_shards(tmp_path, [4, 7, 3])
    cfg = {"batch_size": 4, "image_height": 128, "image_width": 256}
    pipe = augment.TrainPipeline(str(tmp_path), cfg, seed=1, decode=_stub_decode, read_workers=2, epochs=3)
    ids = [int(augment.tfrecords.read_example(r)[0][2:]) for r in pipe.records()]
    assert len(ids) == 3 * total
    for e in range(3):
        assert sorted(ids[e * total:(e + 1) * total]) == list(range(total))
    assert ids[:total] != ids[total:2 * total]
    pipe = augment.TrainPipeline(str(tmp_path), cfg, seed=1, decode=_stub_decode, read_workers=2, epochs=3)
    batches = list(pipe.host_batches())
    assert len(batches) == (3 * total) // 4 and all(len(b) == 4 for b in batches)     # 42 records: 10 batches, 2 dropped
    seen = [int(f[0, 0, 0]) for b in batches for f, _p, _b, _l in b]
    assert seen == ids[:40]


def test_stream_is_the_same_for_any_number_of_readers(tmp_path):
    from ssd_amd import augment
    _write_shards(tmp_path, [9, 6])
    cfg = {"batch_size": 3, "image_height": 128, "image_width": 128}

    def run(workers):
        pipe = augment.TrainPipeline(str(tmp_path), cfg, seed=42, decode=_stub_decode, read_workers=workers, epochs=2)
        return list(pipe.host_batches())
    a, b = run(1), run(8)
    assert len(a) == len(b) == 10
    for ba, bb in zip(a, b):
        for (fa, pa, xa, la), (fb, pb, xb, lb) in zip(ba, bb):
            assert np.array_equal(fa, fb) and pa.tobytes() == pb.tobytes() and np.array_equal(xa, xb) and np.array_equal(la, lb)
    gt = augment.TrainPipeline.groundtruth(a[0])
    assert gt["boxes"].shape == (3, max(1, max(len(l) for *_r, l in a[0])), 4) and gt["num_boxes"].dtype == np.int32


def test_groundtruth_pads_to_one_row_when_no_image_keeps_a_box():
    from ssd_amd import augment
    batch = [(None, None, np.zeros((0, 4), np.float32), np.zeros((0,), np.int32))] * 2
    gt = augment.TrainPipeline.groundtruth(batch)
    assert gt["boxes"].shape == (2, 1, 4) and np.all(gt["boxes"] == 0) and list(gt["num_boxes"]) == [0, 0]


def test_load_train_config():
    from ssd_amd import config
    ref = {"batch_size": 8, "image_height": 640, "image_width": 640, "gamma": 2.0}
    assert config.load_train_config(ref) == {"batch_size": 8, "image_height": 640, "image_width": 640}
    with pytest.raises(ValueError):
        config.load_train_config(dict(ref, image_width=600))
    with pytest.raises(KeyError):
        config.load_train_config({"batch_size": 8, "image_height": 640})


# ----------------------------------------------------------------------------- the C entry point's refusals
def test_ssd_augment_refuses_bad_arguments_without_a_gpu(ssd):
    from ssd_amd import augment
    L = ssd.lib()
    p = np.zeros(2, augment.PARAMS_DTYPE)
    p["height"], p["width"], p["crop_h"], p["crop_w"] = 10, 12, 10, 12
    fake = ctypes.c_void_p(0x10000)           # never dereferenced: every refusal comes before any HIP call

    def call(params=p, images=fake, pdev=fake, B=2, oh=128, ow=256, out=fake):
        return L.ssd_augment(images, params.ctypes.data_as(ctypes.c_void_p) if params is not None else None, pdev, B, oh, ow, 0,
                             out, None)
    for kw in ({"images": None}, {"params": None}, {"pdev": None}, {"out": None}, {"B": 0}, {"oh": 100}, {"ow": 0},
               {"oh": 64}, {"out": ctypes.c_void_p(0x10004)}):
        assert call(**kw) == -1, kw
        assert L.ssd_last_error().decode().startswith("ssd_augment"), kw
    for field, value, word in (("crop_h", 0, "crop window"), ("crop_y", 1, "crop window"), ("crop_x", -1, "crop window"),
                               ("crop_w", 13, "crop window"), ("height", 0, "frame"), ("offset", -4, "frame"),
                               ("flags", 16, "flags")):
        q = p.copy()
        q[1][field] = value
        assert call(params=q) == -1, field
        msg = L.ssd_last_error().decode()
        assert "image 1" in msg and word in msg, (field, msg)
