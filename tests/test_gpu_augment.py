"""The TRAIN input pipeline on the GPU: ssd_augment (csrc/augment.hip) bit for bit against the float32 restatement
(tests/helpers/augment_ref.py) over frame sizes, byte offsets, flags, layouts, output sizes and batch sizes; batch and
stream independence; the statistics of the per-element scale; TrainPipeline end to end into get_training_targets and a few
SGD steps through differentiable_loss."""
import numpy as np
import pytest

from helpers import augment_ref, example_protos

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (7, 5), (33, 17), (127, 129), (375, 500), (480, 640), (640, 640), (641, 333), (300, 1024),
         (1000, 1500), (1280, 720), (129, 1)]
FLAGS = [0, 1, 2, 4, 8, 15]


def _rows(rng, shapes, flags):
    from ssd_amd import augment
    p = np.zeros(len(shapes), augment.PARAMS_DTYPE)
    for b, ((H, W), fl) in enumerate(zip(shapes, flags)):
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        p[b]["height"], p[b]["width"] = H, W
        p[b]["crop_y"], p[b]["crop_x"], p[b]["crop_h"], p[b]["crop_w"] = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
        p[b]["flags"] = fl
        p[b]["color_offset"] = augment.color_offsets(*(rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)))
        p[b]["scale_min"], p[b]["scale_range"] = np.float32(0.85), np.float32(1.15) - np.float32(0.85)
        p[b]["philox_key"] = rng.integers(0, 2 ** 64, dtype=np.uint64)
    return p


def _frames(rng, shapes):
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in shapes]


def _ref(frames, params, hw, cf):
    return np.stack([augment_ref.augment(f, p, hw[0], hw[1], cf) for f, p in zip(frames, params)])


@pytest.mark.parametrize("hw", [(640, 640), (384, 640)])
@pytest.mark.parametrize("cf", [False, True])
def test_kernel_bit_identical_to_the_helper(ssd, cuda, hw, cf):
    rng = np.random.default_rng(hash((hw, cf)) % 2 ** 32)
    shapes = [SIZES[i % len(SIZES)] for i in range(len(SIZES))]
    flags = [FLAGS[i % len(FLAGS)] for i in range(len(shapes))]
    frames, params = _frames(rng, shapes), _rows(rng, shapes, flags)
    got = ssd.augment_batch(frames, params, hw, channels_first=cf).cpu().numpy()
    want = _ref(frames, params, hw, cf)
    assert got.shape == want.shape and got.dtype == np.float32
    for b in range(len(frames)):
        assert np.array_equal(got[b].view(np.uint32), want[b].view(np.uint32)), (b, shapes[b], flags[b])


@pytest.mark.parametrize("B", [1, 7, 64])
def test_every_flag_alone_and_together_over_batch_sizes(ssd, cuda, B):
    rng = np.random.default_rng(B)
    shapes = [SIZES[(3 * i + 1) % len(SIZES)] for i in range(B)]
    flags = [FLAGS[i % len(FLAGS)] if B > 1 else 15 for i in range(B)]
    frames, params = _frames(rng, shapes), _rows(rng, shapes, flags)
    got = ssd.augment_batch(frames, params, (384, 640), channels_first=bool(B % 2)).cpu().numpy()
    want = _ref(frames, params, (384, 640), bool(B % 2))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_device_frames_at_every_byte_offset(ssd, cuda):
    """CUDA frames read where they lie: slices of one buffer starting 0, 1, 2 and 3 bytes past a dword boundary."""
    rng = np.random.default_rng(4)
    shapes = [(33, 17), (7, 5), (480, 640), (129, 1), (375, 500), (2, 3), (127, 129), (641, 333)]
    flags = [15, 0, 4, 8, 1, 2, 12, 15]
    frames, params = _frames(rng, shapes), _rows(rng, shapes, flags)
    sizes = [f.size for f in frames]
    buf = cuda.zeros(sum(sizes) + 64 * len(frames), dtype=cuda.uint8, device="cuda")
    dev, pos = [], 0
    for k, (f, n) in enumerate(zip(frames, sizes)):
        pos = (pos + 3) // 4 * 4 + k % 4                       # byte offset k mod 4 inside its dword
        view = buf[pos:pos + n].view(f.shape)
        view.copy_(cuda.from_numpy(f))
        assert view.data_ptr() % 4 == k % 4 or buf.data_ptr() % 4
        dev.append(view)
        pos += n
    for cf in (False, True):
        got = ssd.augment_batch(dev, params, (640, 640), channels_first=cf).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), _ref(frames, params, (640, 640), cf).view(np.uint32))
        host = ssd.augment_batch(frames, params, (640, 640), channels_first=cf).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


def test_image_does_not_depend_on_batch_position_runs_or_stream(ssd, cuda):
    rng = np.random.default_rng(8)
    shapes = [SIZES[i % len(SIZES)] for i in range(9)]
    frames, params = _frames(rng, shapes), _rows(rng, shapes, [15, 4, 0, 1, 8, 2, 4, 15, 12])
    whole = ssd.augment_batch(frames, params, (384, 640)).cpu().numpy()
    again = ssd.augment_batch(frames, params, (384, 640)).cpu().numpy()
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        other = ssd.augment_batch(frames, params, (384, 640))
    s.synchronize()
    assert np.array_equal(whole.view(np.uint32), other.cpu().numpy().view(np.uint32))
    for b in (0, 4, 8):
        alone = ssd.augment_batch([frames[b]], params[b:b + 1], (384, 640)).cpu().numpy()
        assert np.array_equal(alone[0].view(np.uint32), whole[b].view(np.uint32)), b


def test_pixel_scale_statistics(ssd, cuda):
    """A constant frame that never clips (v = 100/255) with only the scale flag: out / v are the factors drawn."""
    from ssd_amd import augment
    frame = np.full((640, 640, 3), 100, np.uint8)
    p = np.zeros(1, augment.PARAMS_DTYPE)
    p["height"] = p["width"] = p["crop_h"] = p["crop_w"] = 640
    p["flags"], p["philox_key"] = augment.AUG_SCALE, 0x5EED5EED12345678
    p["scale_min"], p["scale_range"] = np.float32(0.85), np.float32(1.15) - np.float32(0.85)
    out = ssd.augment_batch([frame], p, (640, 640)).cpu().numpy().astype(np.float64)
    f = out / float(np.float32(100) * np.float32(1.0 / 255.0))
    assert f.min() >= 0.85 - 1e-6 and f.max() < 1.15 + 1e-6
    assert abs(f.mean() - 1.0) < 1e-3
    assert abs(f.std() - 0.3 / np.sqrt(12)) < 1e-3                     # uniform on [0.85, 1.15)
    assert len(np.unique(out)) > 1000


def test_augment_batch_refuses_bad_windows_and_sizes(ssd, cuda):
    rng = np.random.default_rng(0)
    frames, params = _frames(rng, [(10, 12)]), _rows(rng, [(10, 12)], [0])
    with pytest.raises(ssd.SsdError):
        ssd.augment_batch(frames, params, (100, 128))
    params[0]["crop_h"] = 11
    with pytest.raises(ValueError):
        ssd.augment_batch(frames, params, (128, 128))


# ----------------------------------------------------------------------------- TrainPipeline end to end
def _shard(tmp_path, n=24, seed=0):
    from ssd_amd import tfrecords
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        H, W = int(rng.integers(90, 260)), int(rng.integers(90, 260))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        m = int(rng.integers(1, 4))
        c = rng.uniform(0.1, 0.6, (m, 2))
        boxes = np.concatenate([c, c + rng.uniform(0.15, 0.35, (m, 2))], 1).clip(0, 1)
        recs.append(example_protos.example_bytes(example_protos.jpeg(img), boxes, rng.integers(0, 3, m)))
    tfrecords.write_records(str(tmp_path / "train-00.tfrecords"), recs)
    return str(tmp_path)


CFG = {"batch_size": 4, "image_height": 128, "image_width": 128}


def test_train_pipeline_end_to_end(ssd, cuda, tmp_path):
    path = _shard(tmp_path)
    pipe = ssd.TrainPipeline(path, CFG, seed=3, read_workers=4)
    batches = [next(pipe) for _ in range(3)]
    anchors_np = ssd.AnchorGenerator()(128, 128)
    anchors = cuda.from_numpy(anchors_np).cuda()
    for images, gt in batches:
        assert tuple(images.shape) == (4, 128, 128, 3) and images.dtype == cuda.float32 and images.is_cuda
        assert float(images.min()) >= 0 and float(images.max()) <= 1
        assert set(gt) == {"boxes", "labels", "num_boxes"} and gt["boxes"].is_cuda
        assert gt["boxes"].shape[0] == 4 and gt["boxes"].shape[1] >= 1 and gt["boxes"].shape[2] == 4
        reg, cls, m = ssd.get_training_targets(anchors, gt["boxes"], gt["labels"], gt["num_boxes"])
        assert tuple(reg.shape) == (4, len(anchors_np), 4)
    # the same seed gives the same batches, whatever the readers
    again = ssd.TrainPipeline(path, CFG, seed=3, read_workers=1)
    for images, gt in batches:
        i2, g2 = next(again)
        assert cuda.equal(images, i2) and all(cuda.equal(gt[k], g2[k]) for k in gt)
    cf = next(ssd.TrainPipeline(path, CFG, seed=3, channels_first=True))[0]
    assert cuda.equal(cf, batches[0][0].permute(0, 3, 1, 2))


def test_sgd_through_differentiable_loss_lowers_the_loss(ssd, cuda, tmp_path):
    path = _shard(tmp_path, n=12, seed=1)
    images, gt = next(ssd.TrainPipeline(path, CFG, seed=5, read_workers=2))
    gen = ssd.AnchorGenerator()
    anchors = cuda.from_numpy(gen(128, 128)).cuda()
    levels = list(gen.num_anchors_per_feature_map)
    N, C = int(anchors.shape[0]), 3
    cuda.manual_seed(0)
    model = cuda.nn.Sequential(cuda.nn.Conv2d(3, 8, 3, stride=4, padding=1), cuda.nn.ReLU(), cuda.nn.AdaptiveAvgPool2d(4),
                               cuda.nn.Flatten(), cuda.nn.Linear(128, N * (C + 4))).cuda()
    with cuda.no_grad():
        model[-1].bias[:].view(N, C + 4)[:, :C] = -4.0
    opt = cuda.optim.SGD(model.parameters(), lr=0.5)
    params = {"gamma": 2.0, "alpha": 0.25}
    losses = []
    for _ in range(6):
        out = model(images.permute(0, 3, 1, 2)).view(-1, N, C + 4)
        loss = ssd.differentiable_loss(out[..., :C], out[..., C:], anchors, gt, params, levels)
        total = loss["localization_loss"] + 2.0 * loss["classification_loss"]
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append(total.item())
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses
