"""GPU-side helpers shared by tests/test_gpu_backbone_train.py, tests/test_gpu_shufflenet_train.py, tests/test_gpu_train_scale.py
and tests/test_gpu_shufflenet_train_scale.py: the depthwise and the first convolution's backward (include/ssd_hip.h, "the TRAIN
backbone", "the TRAIN first convolution"; entry "sn_depthwise": "the TRAIN ShuffleNet") through ssd.train_calls on device tensors,
the depthwise tests' data and exact weight gradient, bit equality on the device, and the closed loop of either trainable backbone
through a checkpoint."""
import numpy as np

from helpers import backbone_train_ref as ref
from helpers import head_train_ref as href
from helpers.head_train_gpu import dev, exact_workspace, same_bits

f32 = np.float32


def dw_backward_dev(ssd, cuda, X, Wt, DY, stride, with_dx=True, entry="depthwise"):
    """ssd_depthwise_train_backward (entry "sn_depthwise": ssd_sn_depthwise_train_backward) on device tensors with a workspace of
    exactly the size its planner asks for; the outputs are pre-filled with NaN.  -> (dx or None, dw) on the device."""
    DX = cuda.full_like(X, float("nan")) if with_dx else None
    DW = cuda.full_like(Wt, float("nan"))
    ws = exact_workspace(cuda, ssd.train_calls.depthwise_workspace_bytes(X, stride, entry=entry))
    ssd.train_calls.depthwise_backward(X, Wt, DY, DW, stride, DX, workspace=ws, entry=entry)
    return DX, DW


def dw_backward_raw(ssd, cuda, x, w, dy, stride, with_dx=True, entry="depthwise"):
    """dw_backward_dev on numpy arrays.  -> (dx or None, dw) as numpy."""
    DX, DW = dw_backward_dev(ssd, cuda, dev(cuda, x), dev(cuda, w), dev(cuda, dy), stride, with_dx, entry)
    return DX.cpu().numpy() if with_dx else None, DW.cpu().numpy()


def dw_data(rng, h, w, C, stride, integers=False, batch=2):
    """(x, kernel, dy) of one depthwise layer: normal draws, or small integers whose sums float32 holds exactly."""
    oh, ow = ref.dw_out_hw(h, w, stride)
    if integers:
        return (rng.integers(-3, 4, (batch, h, w, C)).astype(f32), rng.integers(-2, 3, (3, 3, C, 1)).astype(f32),
                rng.integers(-3, 4, (batch, oh, ow, C)).astype(f32))
    return (rng.normal(0, 1, (batch, h, w, C)).astype(f32), rng.normal(0, 0.5, (3, 3, C, 1)).astype(f32),
            rng.normal(0, 1, (batch, oh, ow, C)).astype(f32))


def dw_exact(ssd, cuda, h, w, C, stride, batch, seed, entry="depthwise"):
    """The weight gradient on small integers equals the exact sum.  -> that sum [3,3,C,1] float64."""
    x, k, dy = dw_data(np.random.default_rng(seed), h, w, C, stride, integers=True, batch=batch)
    terms = ref.dw_terms(x, dy, stride)
    assert np.abs(terms).sum(0).max() < 2 ** 24                        # the premise: every partial sum is an exact integer
    want = terms.sum(0).reshape(3, 3, C, 1)
    _, dw = dw_backward_raw(ssd, cuda, x, k, dy, stride, with_dx=False, entry=entry)
    assert dw.shape == k.shape and np.array_equal(dw.astype(np.float64), want), (h, w, C, stride)
    return want


def fc_backward_dev(ssd, cuda, IMG, DY, fill_ws=None):
    """ssd_first_conv_train_backward on device tensors (IMG uint8 [B,H,W,3], DY [B,H/2,W/2,Cout]) with a workspace of exactly the
    planner's size, pre-filled with `fill_ws` (a byte) when given; dw is pre-filled with NaN.  -> dw on the device."""
    DW = cuda.full((3, 3, 3, DY.shape[3]), float("nan"), device="cuda")
    ws = exact_workspace(cuda, ssd.train_calls.first_conv_workspace_bytes(IMG, DY.shape[3]), fill_ws)
    ssd.train_calls.first_conv_backward(IMG, DY, DW, workspace=ws)
    return DW


def same_bits_dev(cuda, a, b):
    """Bit equality of two float32 device tensors (0.0 and -0.0 differ; a NaN equals only the same NaN)."""
    return a.shape == b.shape and cuda.equal(a.contiguous().view(cuda.int32), b.contiguous().view(cuda.int32))


def frames_same_bits(cuda, big, small, ids_dev, chunk=1024):
    """big[b] has the bits of small[ids[b]] for every frame b, compared on the device in chunks of frames.  -> the first chunk's
    start that differs, or None."""
    for b0 in range(0, big.shape[0], chunk):
        if not same_bits_dev(cuda, big[b0:b0 + chunk], small[ids_dev[b0:b0 + chunk]]):
            return b0
    return None


def loop_closes_through_a_checkpoint(ssd, cuda, model_dir, backbone_class, params, frozen_prefix, may_be_zero, level):
    """images -> backbone_class -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward -> one TrainStep over the
    three modules' variables with the first convolution (frozen_prefix) frozen -> save -> a fresh Detector on that checkpoint.
    may_be_zero(variables) -> the names whose gradient may be zero; level: the engine's backbone output ("c3" .. "c5") compared with
    the module's, beside p3."""
    B = 2
    W = ssd.synthetic_weights(params, seed=51, logits_bias=-4.0)
    img = cuda.from_numpy(np.random.default_rng(52).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)).cuda()
    anchors, boxes, labels, num = href.groundtruth(ssd, B, 53)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    backbone = backbone_class(params, W, device="cuda").train()
    fpn = ssd.TrainableFPN(params, W, device="cuda").train()
    head = ssd.TrainableBoxPredictor(params, W, device="cuda").train()
    frozen = backbone.frozen_variables()
    assert len(frozen) == 5 and all(k.startswith(frozen_prefix) for k in frozen)
    cfg = {"initial_learning_rate": 1e-3, "num_steps": 100, "weight_decay": 1e-4}
    variables = {**backbone.named_variables(), **fpn.named_variables(), **head.named_variables()}
    statistics = {**backbone.statistics(), **fpn.statistics(), **head.statistics()}
    assert len(variables) + len(statistics) + len(frozen) == len(W)
    ts = ssd.TrainStep(variables, cfg, statistics, layout="tf", params=params, frozen=frozen)
    eb, cp = head(fpn(backbone(img)))
    out = ssd.differentiable_loss(cp, eb, dev(cuda, anchors), gt, {"gamma": 2.0, "alpha": 0.25})
    (out["localization_loss"] + out["classification_loss"]).backward()
    dead = may_be_zero(variables)
    for name, p in variables.items():
        assert p.grad is not None and bool(cuda.isfinite(p.grad).all()), name
        assert name in dead or float(p.grad.abs().max()) > 0, name
    ts.step()
    ts.save(str(model_dir))
    for name, p in backbone.named_variables().items():
        if name.endswith("weights"):                                    # every backbone kernel has moved
            assert not np.array_equal(p.detach().cpu().numpy(), W[name]), name
    saved = ssd.read_checkpoint(ssd.resolve_checkpoint(str(model_dir)), list(frozen))
    for k, v in frozen.items():
        assert same_bits(saved[k], W[k]) and same_bits(v, W[k]), k
    with cuda.no_grad():
        cs = backbone.eval()(img)
        want_c = cs[int(level[1]) - 3].cpu().numpy()
        want_p3 = fpn.eval()(cs)[0].cpu().numpy()
    det = ssd.Detector(str(model_dir), config=dict(params))
    det.engine.forward(img)
    assert np.array_equal(det.engine.get_tensor(level), want_c) and np.abs(want_c).max() > 0
    assert np.array_equal(det.engine.get_tensor("p3"), want_p3)
    det.close()
