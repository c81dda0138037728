"""The gradient of the EVAL loss on the GPU (loss.hip: ssd_loss_backward) against the float64 helper
(tests/helpers/loss_grad_ref.py) rounded to float32; the autograd op ssd_amd.differentiable_loss; the head outputs of an
Engine end to end; and a few SGD steps through the op."""
import ctypes

import numpy as np
import pytest

from helpers import loss_grad_ref

pytestmark = pytest.mark.gpu

FLT_MIN = np.float32(1.17549435e-38)
LP = {"gamma": 2.0, "alpha": 0.25}


def _gt(anchors, counts, C, seed):
    """[B,G,4] boxes jittered around random anchors (a mix of IoUs, a duplicate gt), labels in [0, C)."""
    rng = np.random.default_rng(seed)
    B, G = len(counts), max(max(counts), 1)
    boxes = np.zeros((B, G, 4), np.float32)
    for b, n in enumerate(counts):
        a = anchors[rng.integers(0, len(anchors), n)].astype(np.float64)
        h, w = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cy = (a[:, 0] + a[:, 2]) / 2 + rng.normal(0, 0.15, n) * h
        cx = (a[:, 1] + a[:, 3]) / 2 + rng.normal(0, 0.15, n) * w
        h, w = h * np.exp(rng.normal(0, 0.3, n)), w * np.exp(rng.normal(0, 0.3, n))
        boxes[b, :n] = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
        if n >= 2:
            boxes[b, 1] = boxes[b, 0]
    return boxes, rng.integers(0, C, (B, G)).astype(np.int32), np.array(counts, np.int32)


def _inputs(ssd, hw, C, counts, seed):
    anchors = ssd.AnchorGenerator()(*hw)
    rng = np.random.default_rng(seed)
    B, N = len(counts), len(anchors)
    logits = rng.normal(-3.0, 3.0, (B, N, C)).astype(np.float32)
    flat = logits.reshape(-1)
    flat[rng.choice(flat.size, min(64, flat.size), replace=False)] = rng.choice([-30.0, 30.0, 0.0, 15.5], min(64, flat.size))
    codes = rng.normal(0.0, 1.5, (B, N, 4)).astype(np.float32)
    boxes, labels, num = _gt(anchors, counts, C, seed)
    return anchors, logits, codes, boxes, labels, num


def _backward(ssd, cuda, logits, codes, anchors, boxes, labels, num, grad, gamma=2.0, alpha=0.25, neg=0.5, offset=0):
    """Targets and per_image on the GPU, then ssd_loss_backward straight through the C ABI into NaN-filled buffers
    (the logits and d_logits `offset` floats past a 16-byte boundary).  Returns numpy (d_logits, d_codes)."""
    L = ssd.lib()
    B, N, C = logits.shape
    a = cuda.from_numpy(anchors).cuda()
    lg_buf = cuda.zeros((B * N * C + 4,), device="cuda")
    lg = lg_buf[offset:offset + B * N * C].view(B, N, C)
    lg.copy_(cuda.from_numpy(logits))
    cd = cuda.from_numpy(codes).cuda()
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    reg, cls, m = ssd.get_training_targets(a, boxes, labels, num, negatives_threshold=neg)
    _, per = ssd.ssd_loss(lg, cd, a, gt, gamma=gamma, alpha=alpha, negatives_threshold=neg)
    dl_buf = cuda.full((B * N * C + 4,), float("nan"), device="cuda")
    dl = dl_buf[offset:offset + B * N * C]
    dc = cuda.full((B, N, 4), float("nan"), device="cuda")
    g = None if grad is None else cuda.tensor(grad, dtype=cuda.float32, device="cuda")
    cfg = ssd.ssd._loss_config(0.5, neg, gamma, alpha, ())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.ssd_loss_backward(p(lg), p(cd), B, N, C, p(reg), p(cls), p(m), p(per), per.shape[1], ctypes.byref(cfg),
                             None if g is None else p(g), p(dl), p(dc), ctypes.c_void_p(cuda.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ssd_last_error()
    cuda.cuda.synchronize()
    return dl.view(B, N, C).cpu().numpy(), dc.cpu().numpy()


def _assert_close(got, want64):
    """Within 1 ulp of the float64 value rounded once, or both below FLT_MIN in magnitude; zeros exact."""
    want = want64.astype(np.float32)
    assert not np.isnan(got).any()
    zero = want64 == 0
    assert np.array_equal(got[zero], want[zero])
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    ok = (ulp <= 1) | ((np.abs(got) < FLT_MIN) & (np.abs(want) < FLT_MIN))
    assert ok.all(), (np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])


@pytest.mark.parametrize("C,grad,gamma,alpha,neg,offset", [
    (80, None, 2.0, 0.25, 0.5, 0),
    (80, (1.0, 2.0), 2.0, 0.25, 0.4, 1),            # misaligned rows: the one-per-thread path; ignored anchors
    (7, (1.0, 2.0), 2.0, 0.25, 0.5, 0),
    (3, (0.0, -3.5), 1.5, 0.3, 0.4, 0),
    (1, (1.0, 2.0), 2.0, 0.25, 0.5, 0),
])
def test_kernel_against_helper(ssd, cuda, C, grad, gamma, alpha, neg, offset):
    anchors, logits, codes, boxes, labels, num = _inputs(ssd, (128, 256), C, [3, 0, 300, 17], seed=C + offset)
    dl, dc = _backward(ssd, cuda, logits, codes, anchors, boxes, labels, num, grad, gamma, alpha, neg, offset)
    w_l, w_c = loss_grad_ref.batch_grads(logits, codes, anchors, boxes, labels, num, gamma, alpha,
                                         (1.0, 1.0) if grad is None else grad, 0.5, neg)
    _assert_close(dl, w_l)
    _assert_close(dc, w_c)
    assert np.count_nonzero(dl) > dl.size // 2
    assert not dc[1].any()                                                  # the image without gt: no positive anchor
    assert (np.count_nonzero(dc) == 0) == (grad is not None and grad[0] == 0.0)  # g_loc = 0: every d_codes zero


def test_two_calls_and_another_stream_give_the_same_bits(ssd, cuda):
    anchors, logits, codes, boxes, labels, num = _inputs(ssd, (128, 256), 80, [5, 40], seed=3)
    args = (logits, codes, anchors, boxes, labels, num, (1.0, 2.0))
    first = _backward(ssd, cuda, *args)
    again = _backward(ssd, cuda, *args)
    s = cuda.cuda.Stream()
    s.wait_stream(cuda.cuda.current_stream())
    with cuda.cuda.stream(s):
        other = _backward(ssd, cuda, *args)
    for x, y, z in zip(first, again, other):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)) and np.array_equal(x.view(np.int32), z.view(np.int32))


def test_autograd_matches_the_entry_point(ssd, cuda):
    g = ssd.AnchorGenerator()
    anchors, logits, codes, boxes, labels, num = _inputs(ssd, (128, 256), 80, [4, 0, 9], seed=8)
    g(128, 256)
    levels = g.num_anchors_per_feature_map
    a = cuda.from_numpy(anchors).cuda()
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    lg = cuda.from_numpy(logits).cuda().requires_grad_(True)
    cd = cuda.from_numpy(codes).cuda().requires_grad_(True)
    out = ssd.differentiable_loss(lg, cd, a, gt, LP, anchors_per_level=levels)
    assert out["localization_loss"].dim() == 0 and out["classification_loss"].dim() == 0
    losses, per = ssd.ssd_loss(lg.detach(), cd.detach(), a, gt, anchors_per_level=levels)
    assert out["localization_loss"].item() == losses[0].item() and out["classification_loss"].item() == losses[1].item()
    (1.0 * out["localization_loss"] + 2.0 * out["classification_loss"]).backward()
    reg, cls, m = ssd.get_training_targets(a, boxes, labels, num)
    d_l, d_c = ssd.ssd_loss_backward(lg.detach(), cd.detach(), reg, cls, m, per, grad_losses=(1.0, 2.0))
    assert cuda.equal(lg.grad, d_l) and cuda.equal(cd.grad, d_c)
    assert a.grad is None
    # a non-contiguous input is copied; its gradient has the input's shape and the same values
    lt = cuda.from_numpy(np.ascontiguousarray(logits.transpose(0, 2, 1))).cuda().requires_grad_(True)
    out2 = ssd.differentiable_loss(lt.transpose(1, 2), cd.detach(), a, gt, LP, anchors_per_level=levels)
    (out2["localization_loss"] + 2.0 * out2["classification_loss"]).backward()
    assert cuda.equal(lt.grad.transpose(1, 2), d_l)
    # only one loss used: the other's gradient is zero
    lg.grad = None
    cd.grad = None
    ssd.differentiable_loss(lg, cd, a, gt, LP)["classification_loss"].backward()
    d_l1, _ = ssd.ssd_loss_backward(lg.detach(), cd.detach(), reg, cls, m, per, grad_losses=(0.0, 1.0))
    assert cuda.equal(lg.grad, d_l1) and not cd.grad.any()


def _params(backbone):
    return {"backbone": backbone, "depth_multiplier": 1.0 if backbone == "mobilenet" else 0.5, "num_classes": 80,
            "score_threshold": 0.15, "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 640}


@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_engine_head_outputs_end_to_end(ssd, cuda, backbone):
    params = _params(backbone)
    eng = ssd.Engine(params, ssd.synthetic_weights(params, seed=6, logits_bias=-3.0), device=0, precision="f32")
    imgs = np.random.default_rng(2).integers(0, 256, (2, 640, 896, 3), dtype=np.uint8)     # bench.py's network shape
    model = ssd.SSD(cuda.from_numpy(imgs).cuda(), eng)
    lg, cd = model.raw_predictions["class_predictions"], model.raw_predictions["encoded_boxes"]
    anchors = model.anchors.cpu().numpy()
    boxes, labels, num = _gt(anchors, [12, 5], 80, seed=4)
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    x = lg.clone().requires_grad_(True)
    c = cd.clone().requires_grad_(True)
    out = ssd.differentiable_loss(x, c, model.anchors, gt, LP, anchors_per_level=model.num_anchors_per_feature_map)
    (out["localization_loss"] + out["classification_loss"]).backward()
    ref = model.loss(gt, LP)
    assert out["localization_loss"].item() == ref["localization_loss"].item()
    assert out["classification_loss"].item() == ref["classification_loss"].item()
    assert lg.shape == (2, 71610, 80)
    w_l, w_c = loss_grad_ref.batch_grads(lg.cpu().numpy(), cd.cpu().numpy(), anchors, boxes, labels, num)
    _assert_close(x.grad.cpu().numpy(), w_l)
    _assert_close(c.grad.cpu().numpy(), w_c)
    eng.close()


def test_sgd_steps_through_the_op_decrease_the_loss(ssd, cuda):
    anchors, logits, codes, boxes, labels, num = _inputs(ssd, (128, 256), 80, [6, 2], seed=12)
    a = cuda.from_numpy(anchors).cuda()
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    lg = cuda.nn.Parameter(cuda.from_numpy(logits).cuda())
    cd = cuda.nn.Parameter(cuda.from_numpy(codes).cuda())
    _, per = ssd.ssd_loss(lg.detach(), cd.detach(), a, gt)
    norm = max(float(per[:, 2].sum().item()), 1.0)
    opt = cuda.optim.SGD([lg, cd], lr=0.5 * norm)                 # the per-element curvature is at most ~1 / norm
    totals = []
    for _ in range(20):
        opt.zero_grad()
        out = ssd.differentiable_loss(lg, cd, a, gt, LP)
        total = out["localization_loss"] + out["classification_loss"]
        total.backward()
        opt.step()
        totals.append(total.item())
    assert all(b < a_ for a_, b in zip(totals, totals[1:])), totals
    assert totals[-1] < 0.5 * totals[0], totals
