"""The training loop from the batches the library itself produces:

    TrainPipeline -> TrainableMobileNet(train_first=True) -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward
                  -> TrainStep.step(), twice -> save -> Detector

on a tiny .tfrecords shard (test_gpu_augment.py's writer, restated), and one iteration with TrainableShuffleNet(train_first=True).
The batches are float32 frames that are NOT on the byte grid, so the first convolution runs first_conv_train_float on values no uint8
frame can carry."""
import numpy as np
import pytest

from helpers import example_protos
from helpers import first_conv_f32_ref as ref
from helpers import head_train_ref as href
from helpers import shufflenet_train_ref as sref
from helpers.head_train_gpu import same_bits
from conftest import TINY_PARAMS

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
CFG = {"batch_size": 2, "image_height": 128, "image_width": 128}
OPT = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
LP = {"gamma": 2.0, "alpha": 0.25}
# The pipeline's seed.  Colour offsets and the per-element scale have probability 0.05 each (pipeline.py:120-135; crop, nearest-neighbour
# resize and flip keep a frame on the byte grid), so most batches of two ARE on it: 36 is the first seed -- found on the CPU through
# host_batches -- whose first two batches each hold an image that takes colour offsets or the scale (batch 0: one of each; batch 1:
# colour offsets) and every image of whose first three batches keeps a box.  Both premises are asserted below.
SEED = 36
SN_PARAMS = dict(TINY_PARAMS, backbone="shufflenet")


def _shard(tmp_path, n=24, seed=0):
    """test_gpu_augment.py's shard: n JPEGs of random sizes with 1 .. 3 boxes each."""
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
    d = tmp_path / "shard"
    d.mkdir()
    tfrecords.write_records(str(d / "train-00.tfrecords"), recs)
    return str(d)


def _premises(ssd, path, n_batches, n_used):
    """On the CPU, through sample_augmentation (TrainPipeline.host_batches): every image of the first batches keeps a box, and each
    batch that is used holds an image with colour offsets or the per-element scale."""
    from ssd_amd import augment
    host = ssd.TrainPipeline(path, CFG, seed=SEED, read_workers=2).host_batches()
    for i in range(n_batches):
        batch = next(host)
        kept = [len(labels) for _frame, _row, _boxes, labels in batch]
        assert len(kept) == 2 and min(kept) >= 1, kept
        flags = [int(row["flags"]) for _frame, row, _boxes, _labels in batch]
        assert i >= n_used or any(f & (augment.AUG_COLOR | augment.AUG_SCALE) for f in flags), (i, flags)
    host.close()


def _off_the_byte_grid(images):
    """How many elements of the float batch are no fp32(u * inv255)."""
    x = images.cpu().numpy()
    assert x.dtype == f32 and x.min() >= 0 and x.max() <= 1
    return int((~np.isin(x, ref.byte_frames(np.arange(256, dtype=np.uint8)))).sum()), x


def _hook_first_conv(monkeypatch, module, captured):
    """The raw first convolution's output gradient -- the dy that reaches Conv2d_0 / Conv1 -- lands in `captured`."""
    inner = module.first_conv_train_float

    def hooked(images, kernel):
        y = inner(images, kernel)
        if y.requires_grad:
            y.register_hook(lambda g: captured.append(g.detach().clone()))
        return y
    monkeypatch.setattr(module, "first_conv_train_float", hooked)


def _modules(ssd, params, backbone_cls, W):
    backbone = getattr(ssd, backbone_cls)(params, W, device="cuda", train_first=True).train()
    fpn = ssd.TrainableFPN(params, W, device="cuda").train()
    head = ssd.TrainableBoxPredictor(params, W, device="cuda").train()
    assert backbone.frozen_variables() == {}
    variables = {**backbone.named_variables(), **fpn.named_variables(), **head.named_variables()}
    statistics = {**backbone.statistics(), **fpn.statistics(), **head.statistics()}
    assert len(variables) + len(statistics) == len(W)
    ts = ssd.TrainStep(variables, OPT, statistics, layout="tf", params=params, frozen={})
    return backbone, fpn, head, variables, ts


def _levels_without_a_match(ssd, cuda, anchors, gt):
    """The pyramid levels (3 .. 7) none of whose anchors is matched to a box in this batch, from ssd_training_targets -- the matching
    the loss itself uses, pinned by the loss tests.  At 128 x 128 the anchors of p6 and p7 are 1.4 .. 8 times the image, and the
    pipeline clips every box to the image, so IoU with them stays below 1/2 and no forced match lands there: the localization loss
    has no term on such a level, and the gradient of box_net's batch norms FOR THAT LEVEL is zero in exact arithmetic -- and here
    exactly 0.0, since every contribution is a product with a zero upstream gradient.  (class_net's per-level batch norms are
    reached by the focal loss of the negatives on every level.)"""
    _reg, _cls, matches = ssd.get_training_targets(anchors, gt["boxes"], gt["labels"], gt["num_boxes"])
    g = ssd.AnchorGenerator()
    g(128, 128)
    per_level, at, silent = list(g.num_anchors_per_feature_map), 0, []
    assert len(per_level) == 5 and sum(per_level) == matches.shape[1]
    for level, n in zip(range(3, 8), per_level):
        if not bool((matches[:, at:at + n] >= 0).any()):
            silent.append(level)
        at += n
    return silent


def _iteration(ssd, cuda, images, gt, anchors, backbone, fpn, head, variables, dead=()):
    """One forward, loss and backward.  Every gradient is finite; every gradient is non-zero except those that are zero in exact
    arithmetic: `dead` (ShuffleNet's 19 depthwise betas, finite only) and box_net's batch norms of the levels without a matched
    anchor, which must be exactly zero -- the set is derived from the matching, not from the gradients."""
    for p in variables.values():
        p.grad = None
    silent = _levels_without_a_match(ssd, cuda, anchors, gt)
    assert 3 not in silent                                               # p3 holds matches: the localization loss is live
    print("levels without a matched anchor: %s" % silent)
    zero = {"box_net/batch_norm_%d_for_level_%d/%s" % (i, l, leaf) for i in range(4) for l in silent for leaf in ("gamma", "beta")}
    assert zero <= set(variables)
    eb, cp = head(fpn(backbone(images)))
    out = ssd.differentiable_loss(cp, eb, anchors, gt, LP)
    loss = out["localization_loss"] + out["classification_loss"]
    loss.backward()
    assert np.isfinite(float(out["localization_loss"].detach())) and np.isfinite(float(out["classification_loss"].detach()))
    assert float(out["localization_loss"].detach()) > 0 and float(out["classification_loss"].detach()) > 0
    for name, p in variables.items():
        assert p.grad is not None and bool(cuda.isfinite(p.grad).all()), name
        if name in zero:
            assert float(p.grad.abs().max()) == 0, name
        else:
            assert name in dead or float(p.grad.abs().max()) > 0, name
    return float(loss.detach())


def _first_dw_check(x, dy, dw, tag):
    """dw [3,3,3,Cout] against the float64 sum of q(x) * dy over the batch, within head_train_ref.double_sum_bound."""
    terms = ref.fc_terms(x, dy)
    Cout = dy.shape[3]
    worst = 0.0
    for t in range(27):
        want, tol = href.double_sum_bound(terms[:, t, :])
        err = np.abs(dw.reshape(27, Cout)[t].astype(f64) - want.astype(f64))
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (tag, t, float((err / tol).max()))
    print("%s: d first kernel from the pipeline's frames, worst |dw - exact| / bound = %.3g" % (tag, worst))


def test_the_loop_runs_from_the_pipelines_float_batches(ssd, cuda, tmp_path, monkeypatch):
    FIRST = "MobilenetV1/Conv2d_0"
    path = _shard(tmp_path)
    _premises(ssd, path, 3, 2)                                            # two batches are used, a third is prefetched
    pipe = ssd.TrainPipeline(path, CFG, seed=SEED, read_workers=2)
    W = ssd.synthetic_weights(TINY_PARAMS, seed=201, logits_bias=-4.0)
    backbone, fpn, head, variables, ts = _modules(ssd, TINY_PARAMS, "TrainableMobileNet", W)
    anchors = cuda.from_numpy(ssd.AnchorGenerator()(128, 128)).cuda()
    captured = []
    _hook_first_conv(monkeypatch, ssd.backbone_train, captured)
    losses = []
    for it in range(2):
        images, gt = next(pipe)
        assert tuple(images.shape) == (2, 128, 128, 3) and images.dtype == cuda.float32 and int(gt["num_boxes"].min()) >= 1
        off, x = _off_the_byte_grid(images)
        assert off > 0                                                   # the premise: no uint8 frame carries this batch
        print("batch %d: %d of %d elements off the byte grid" % (it, off, x.size))
        losses.append(_iteration(ssd, cuda, images, gt, anchors, backbone, fpn, head, variables))
        if it == 0:
            assert len(captured) == 1 and tuple(captured[0].shape) == (2, 64, 64, 32)
            _first_dw_check(x, captured[0].cpu().numpy(), variables[FIRST + "/weights"].grad.cpu().numpy(), "mobilenet")
        ts.step()
    assert np.all(np.isfinite(losses)), losses
    ts.save(str(tmp_path))
    first = [FIRST + "/weights", FIRST + "/BatchNorm/gamma", FIRST + "/BatchNorm/beta", FIRST + "/BatchNorm/moving_mean",
             FIRST + "/BatchNorm/moving_variance"]
    now = {**backbone.named_variables(), **backbone.statistics()}
    saved = ssd.read_checkpoint(ssd.resolve_checkpoint(str(tmp_path)), first)
    for k in first:                                                     # Conv2d_0 moved, and the checkpoint holds what it moved to
        assert not same_bits(now[k].detach().cpu().numpy(), W[k]), k
        assert same_bits(saved[k], now[k].detach().cpu().numpy()), k
    frame = cuda.from_numpy(np.random.default_rng(202).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)).cuda()
    with cuda.no_grad():
        cs = backbone.eval()(frame)
        want_c5 = cs[2].cpu().numpy()
        want_p3 = fpn.eval()(cs)[0].cpu().numpy()
    det = ssd.Detector(str(tmp_path), config=dict(TINY_PARAMS))
    det.engine.forward(frame)
    assert np.array_equal(det.engine.get_tensor("c5"), want_c5) and np.abs(want_c5).max() > 0
    assert np.array_equal(det.engine.get_tensor("p3"), want_p3)
    det.close()


def test_one_shufflenet_iteration_from_the_pipeline(ssd, cuda, tmp_path, monkeypatch):
    """The 19 betas of the depthwise batch norms have a gradient that is zero in exact arithmetic: finite only."""
    FIRST = "ShuffleNetV2/Conv1"
    path = _shard(tmp_path)
    _premises(ssd, path, 2, 1)
    pipe = ssd.TrainPipeline(path, CFG, seed=SEED, read_workers=2)
    W = ssd.synthetic_weights(SN_PARAMS, seed=211, logits_bias=-4.0)
    backbone, fpn, head, variables, ts = _modules(ssd, SN_PARAMS, "TrainableShuffleNet", W)
    dead = sref.dead_betas(variables)
    assert len(dead) == 19
    anchors = cuda.from_numpy(ssd.AnchorGenerator()(128, 128)).cuda()
    captured = []
    _hook_first_conv(monkeypatch, ssd.backbone_train, captured)      # TrainableBackbone.first_conv looks the op up there
    images, gt = next(pipe)
    off, x = _off_the_byte_grid(images)
    assert off > 0 and int(gt["num_boxes"].min()) >= 1
    loss = _iteration(ssd, cuda, images, gt, anchors, backbone, fpn, head, variables, dead)
    assert np.isfinite(loss)
    assert len(captured) == 1 and tuple(captured[0].shape) == (2, 64, 64, 24)
    _first_dw_check(x, captured[0].cpu().numpy(), variables[FIRST + "/weights"].grad.cpu().numpy(), "shufflenet")
    ts.step()
    now = {**backbone.named_variables(), **backbone.statistics()}
    for leaf in ("weights", "batch_norm/gamma", "batch_norm/beta", "batch_norm/moving_mean", "batch_norm/moving_variance"):
        assert not same_bits(now[FIRST + "/" + leaf].detach().cpu().numpy(), W[FIRST + "/" + leaf]), leaf
