"""The gradient of the EVAL loss, host side (no GPU): the float64 helper (tests/helpers/loss_grad_ref.py) against torch
autograd of an independent float64 restatement of losses.py, against central differences of loss_ref.losses_f64, and
against hand-worked values; ssd_loss_backward's argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import loss_grad_ref, loss_ref

f32 = np.float32


def _case(seed, B=3, C=3, pos=0.5, neg=0.4):
    """A small batch: anchors on a 2-scale grid, image 0 with several gt (positives, negatives and -- pos != neg -- ignored
    anchors), image 1 with none, image 2 with one; logits with the extremes +-30 and codes within +-1 of the targets and
    beyond."""
    rng = np.random.default_rng(seed)
    cells = []
    for size in (0.25, 0.5):
        for cy in np.arange(size / 2, 1.0, size / 2):
            for cx in np.arange(size / 2, 1.0, size / 2):
                cells.append([cy - size / 2, cx - size / 2, cy + size / 2, cx + size / 2])
    anchors = np.array(cells, f32)
    N = len(anchors)
    G = 4
    boxes = np.zeros((B, G, 4), f32)
    boxes[0, :4] = [[0.0, 0.0, 0.3, 0.3], [0.1, 0.4, 0.6, 0.9], [0.5, 0.5, 1.0, 1.0], [0.05, 0.6, 0.25, 0.95]]
    boxes[2, :1] = [[0.2, 0.2, 0.7, 0.75]]
    labels = rng.integers(0, C, (B, G)).astype(np.int32)
    num = np.array([4, 0, 1], np.int32)[:B]
    logits = rng.normal(-1.0, 3.0, (B, N, C)).astype(f32)
    flat = logits.reshape(-1)
    flat[rng.choice(flat.size, 12, replace=False)] = rng.choice([-30.0, 30.0, -12.5, 17.0], 12)
    reg = np.stack([loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]], pos, neg)[0] for b in range(B)])
    codes = (reg + rng.uniform(-2.5, 2.5, reg.shape)).astype(f32)
    one = (reg + f32(1.0)) - reg == f32(1.0)                                      # |diff| exactly 1 where that is exact
    codes[:, ::3][one[:, ::3]] = (reg + f32(1.0))[:, ::3][one[:, ::3]]
    codes[:, 1::5][one[:, 1::5]] = (reg - f32(1.0))[:, 1::5][one[:, 1::5]]
    return anchors, boxes, labels, num, logits, codes


def _targets(anchors, boxes, labels, num, pos, neg):
    return [loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]], pos, neg) for b in range(len(num))]


def _torch_grads(logits, codes, targets, gamma, alpha, grad):
    """torch.autograd of losses.py / ssd.py:71-133 restated in float64 torch ops on the targets: 1 - sigmoid(x) as
    sigmoid(-x) and -log p_t as softplus, so the restatement has no cancellation of its own."""
    B, N, C = logits.shape
    x = torch.tensor(logits.astype(np.float64), requires_grad=True)
    diff_np = np.stack([codes[b] - targets[b][0] for b in range(B)]).astype(np.float64)        # one fp32 op, as the kernel
    diff = torch.tensor(diff_np, requires_grad=True)                                         # d/d codes == d/d diff
    cls = torch.tensor(np.stack([t[1] for t in targets]).astype(np.int64))
    m = torch.tensor(np.stack([t[2] for t in targets]).astype(np.int64))
    z = torch.nn.functional.one_hot(cls, C + 1)[:, :, 1:].bool()
    a, oma = float(f32(alpha)), float(f32(1.0 - alpha))
    sp = lambda v: torch.nn.functional.softplus(v, beta=1.0, threshold=1000.0)
    fl = torch.where(z, a * torch.sigmoid(-x) ** gamma * sp(-x), oma * torch.sigmoid(x) ** gamma * sp(x))
    cls_loss = (fl.sum(2) * (m >= -1).double()).sum()
    ad = diff.abs()
    sl = torch.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5)
    loc_loss = (sl.sum(2) * (m >= 0).double()).sum()
    norm = float(max(f32(int((m >= 0).sum())), f32(1)))
    total = float(f32(grad[0])) * loc_loss / norm + float(f32(grad[1])) * cls_loss / norm
    total.backward()
    return x.grad.numpy(), diff.grad.numpy()


@pytest.mark.parametrize("seed,C,gamma,alpha,grad", [(0, 3, 2.0, 0.25, (1.0, 1.0)), (1, 7, 2.0, 0.25, (1.0, 2.0)),
                                                     (2, 1, 1.5, 0.3, (0.0, -3.5)), (3, 3, 0.5, 0.25, (2.0, 0.5))])
def test_helper_equals_torch_autograd(seed, C, gamma, alpha, grad):
    anchors, boxes, labels, num, logits, codes = _case(seed, C=C)
    pos, neg = 0.5, 0.4
    targets = _targets(anchors, boxes, labels, num, pos, neg)
    ms = np.stack([t[2] for t in targets])
    assert (ms >= 0).any() and (ms == -1).any() and (ms == -2).any()                   # positives, negatives, ignored
    d_logits, d_codes = loss_grad_ref.batch_grads(logits, codes, anchors, boxes, labels, num, gamma, alpha, grad, pos, neg)
    t_logits, t_codes = _torch_grads(logits, codes, targets, gamma, alpha, grad)
    np.testing.assert_allclose(d_logits, t_logits, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(d_codes, t_codes, rtol=1e-12, atol=1e-300)
    # ignored anchors and the codes of unmatched anchors: exactly 0; an image without gt: codes all 0
    assert not d_logits[ms == -2].any() and not d_codes[ms < 0].any()
    diff = np.stack([codes[b] - targets[b][0] for b in range(len(num))])
    on = (ms >= 0)[:, :, None] & np.ones((1, 1, 4), bool)
    assert (on & (np.abs(diff) < 1)).any() and (on & (np.abs(diff) > 1)).any() and (on & (np.abs(diff) == 1)).any()


def test_helper_equals_central_differences():
    anchors, boxes, labels, num, logits, codes = _case(7, C=3)
    grad = (1.0, 2.0)
    d_logits, d_codes = loss_grad_ref.batch_grads(logits, codes, anchors, boxes, labels, num, grad=grad)
    x64, c64 = logits.astype(np.float64), codes.astype(np.float64)
    f = lambda lg, cd: float(np.dot(grad, loss_ref.losses_f64(lg, cd, anchors, boxes, labels, num)))
    tol = lambda d: 1e-6 * abs(d) + 1e-8              # + the rounding of the summed loss (~1e-14) over 2h
    rng = np.random.default_rng(1)
    h = 1e-5
    idx = [np.unravel_index(i, logits.shape) for i in rng.choice(logits.size, 40, replace=False)]
    idx += [np.unravel_index(i, logits.shape) for i in np.flatnonzero(np.abs(logits) >= 12)[:6]]
    for i in idx:
        p, m = x64.copy(), x64.copy()
        p[i] += h
        m[i] -= h
        fd = (f(p, c64) - f(m, c64)) / (2 * h)
        assert abs(fd - d_logits[i]) <= tol(d_logits[i]), (i, fd, d_logits[i])
    matched = np.argwhere(np.stack([t[2] for t in _targets(anchors, boxes, labels, num, 0.5, 0.5)]) >= 0)
    assert len(matched) > 0
    reg = np.stack([t[0] for t in _targets(anchors, boxes, labels, num, 0.5, 0.5)])
    for b, a in list(matched[:8]) + [(1, 0)]:
        for k in range(4):
            i = (b, a, k)
            if abs(abs(float(codes[i]) - float(reg[i])) - 1.0) < 2 * h:
                continue                                                     # the kink of smooth-L1's second derivative
            p, m = c64.copy(), c64.copy()
            p[i] += h
            m[i] -= h
            fd = (f(x64, p) - f(x64, m)) / (2 * h)
            assert abs(fd - d_codes[i]) <= tol(d_codes[i]), (i, fd, d_codes[i])


def test_hand_worked_values():
    # x = 0, z = 1, gamma = 2, alpha = 0.25: s = q = 1/2, dq/dx = -1/4, nlp = ln 2
    assert math.isclose(loss_grad_ref.focal_grad(0.0, True)[()], 0.25 * (-0.25 * math.log(2) - 0.125), rel_tol=1e-15)
    # z = 0: s = q = 1/2, dq/dx = +1/4, (1 - alpha) = 0.75
    assert math.isclose(loss_grad_ref.focal_grad(0.0, False)[()], 0.75 * (0.25 * math.log(2) + 0.125), rel_tol=1e-15)
    # smooth-L1: diff inside (the diff itself), exactly +-1 (sign: tf.less is false there), beyond (sign)
    codes = np.array([0.5, 1.0, -1.0, -2.0, 3.0], f32)
    assert loss_grad_ref.smooth_l1_grad(codes, np.zeros(5, f32)).tolist() == [0.5, 1.0, -1.0, -1.0, 1.0]
    # gamma < 1 where q == 0 (x = +800, z = 1: exp(-x), so 1 - sigma(x), is 0 in double): the first term is 0, not inf * 0
    assert loss_grad_ref.focal_grad(800.0, True, gamma=0.5)[()] == 0.0


def test_loss_backward_refuses_bad_arguments_without_a_gpu(ssd):
    """ssd_loss_backward checks its arguments before any HIP call (include/ssd_hip.h); every call below has one defect."""
    L = ssd.lib()
    cfg = ssd.ssd._loss_config(0.5, 0.5)
    P = lambda a: ctypes.c_void_p(a)
    good = dict(lg=P(0x10000), cd=P(0x20000), B=2, N=10, C=80, reg=P(0x30000), cls=P(0x40000), m=P(0x50000), per=P(0x60000),
                stride=3, cfg=ctypes.byref(cfg), g=None, dl=P(0x70000), dc=P(0x80000))
    defects = [dict(lg=None), dict(cd=None), dict(reg=None), dict(cls=None), dict(m=None), dict(per=None), dict(cfg=None),
               dict(dl=None), dict(dc=None), dict(B=0), dict(N=0), dict(C=0), dict(C=(1 << 22) + 1), dict(stride=2),
               dict(cd=P(0x20004)), dict(reg=P(0x30008)), dict(dc=P(0x8000c)), dict(lg=P(0x10002)), dict(dl=P(0x70001)),
               dict(per=P(0x60002)), dict(g=P(0x90003)), dict(cls=P(0x40002)), dict(B=1 << 20, N=1 << 20)]
    for d in defects:
        a = dict(good, **d)
        rc = L.ssd_loss_backward(a["lg"], a["cd"], a["B"], a["N"], a["C"], a["reg"], a["cls"], a["m"], a["per"], a["stride"],
                                 a["cfg"], a["g"], a["dl"], a["dc"], None)
        assert rc == -1, d                                                     # SSD_ERR_INVALID
        assert b"ssd_loss_backward" in L.ssd_last_error(), d
