"""Float64 numpy restatement of the TRAIN head (include/ssd_hip.h, "the TRAIN head"): the 3x3 'same' convolution and the
training-mode batch norm + ReLU with their gradients, and the whole RetinaNetBoxPredictor (box_predictor.py:34-155) forward and
backward; plus the float32 restatement of the batch norm in the header's operation order."""
import numpy as np

EPS = 1e-3
MOMENTUM = 0.993
f32 = np.float32


def _shifted(x, kh, kw):
    """x [B,H,W,C] -> the tensor a 'same' 3x3 tap (kh, kw) reads: x[b, y+kh-1, x+kw-1], zero outside."""
    B, H, W, C = x.shape
    p = np.zeros((B, H + 2, W + 2, C), x.dtype)
    p[:, 1:H + 1, 1:W + 1] = x
    return p[:, kh:kh + H, kw:kw + W]


def conv3x3(x, w, bias=None):
    y = np.zeros(x.shape[:3] + (w.shape[3],), np.float64)
    for kh in range(3):
        for kw in range(3):
            y += _shifted(x.astype(np.float64), kh, kw) @ w[kh, kw].astype(np.float64)
    return y if bias is None else y + bias.astype(np.float64)


def conv3x3_grads(xs, w, dys, absolute=False):
    """Levels xs, dys -> ([dx per level], dw, dbias).  absolute=True: the sums of |x * dy| per dw element instead of dw."""
    w = w.astype(np.float64)
    dw = np.zeros(w.shape, np.float64)
    db = np.zeros(w.shape[3], np.float64)
    dxs = []
    for x, dy in zip(xs, dys):
        x, dy = x.astype(np.float64), dy.astype(np.float64)
        dx = np.zeros(x.shape, np.float64)
        B, H, W, _ = x.shape
        pad = np.zeros((B, H + 2, W + 2, x.shape[3]), np.float64)
        for kh in range(3):
            for kw in range(3):
                xs_ = _shifted(x, kh, kw)
                a2, d2 = xs_.reshape(-1, xs_.shape[3]), dy.reshape(-1, dy.shape[3])
                dw[kh, kw] += np.abs(a2).T @ np.abs(d2) if absolute else a2.T @ d2
                pad[:, kh:kh + H, kw:kw + W] += dy @ w[kh, kw].T
        dx = pad[:, 1:H + 1, 1:W + 1]
        db += dy.sum((0, 1, 2))
        dxs.append(dx)
    return dxs, dw, db


def rotated_transposed(w):
    """w'[kh,kw,co,ci] = w[2-kh,2-kw,ci,co]: the data gradient is conv3x3_same(dy, w')."""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def bn_relu_forward(x, gamma, beta, eps=EPS):
    """x [..., C] float64 -> y, mean, var (biased), invstd."""
    x2 = x.reshape(-1, x.shape[-1]).astype(np.float64)
    mean = x2.mean(0)
    var = ((x2 - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    y = np.maximum((x.astype(np.float64) - mean) * (gamma * invstd) + beta, 0.0)
    return y, mean, var, invstd


def bn_relu_backward(x, gamma, beta, dy, eps=EPS):
    y, mean, var, invstd = bn_relu_forward(x, gamma, beta, eps)
    R = x.size // x.shape[-1]
    g = np.where(y > 0, dy.astype(np.float64), 0.0)
    xh = (x.astype(np.float64) - mean) * invstd
    ax = tuple(range(x.ndim - 1))
    dbeta = g.sum(ax)
    dgamma = (g * xh).sum(ax)
    dx = gamma * invstd * (g - dbeta / R - xh * dgamma / R)
    return dx, dgamma, dbeta


def moving_update(moving_mean, moving_variance, mean, var, rows, momentum=MOMENTUM):
    """float32, the header's order: moving -= (moving - batch) * fp32(1 - momentum), unbiased variance."""
    omm = f32(1.0 - momentum)
    unbias = f32(rows / (rows - 1.0)) if rows > 1 else f32(1.0)
    mm = moving_mean - (moving_mean - mean) * omm
    mv = moving_variance - (moving_variance - var * unbias) * omm
    return mm.astype(f32), mv.astype(f32)


def invstd_f32(var, eps=EPS):
    return (f32(1.0) / np.sqrt(var.astype(f32) + f32(eps))).astype(f32)


def bn_relu_f32(x, gamma, beta, mean, var, dy=None, dgamma=None, dbeta=None, eps=EPS):
    """The header's float32 operation sequence on given float32 statistics: y, and with dy also dgamma, dbeta (float32
    accumulation in numpy's order unless given) and dx."""
    x, gamma, beta, mean = (v.astype(f32) for v in (x, gamma, beta, mean))
    invstd = invstd_f32(var, eps)
    t = x - mean
    sf = gamma * invstd
    ypre = t * sf + beta
    y = np.where(ypre > 0, ypre, f32(0))
    if dy is None:
        return y
    R = f32(x.size // x.shape[-1])
    xh = t * invstd
    g = np.where(ypre > 0, dy.astype(f32), f32(0))
    ax = tuple(range(x.ndim - 1))
    if dbeta is None:
        dbeta = g.sum(ax, dtype=f32)
        dgamma = (g * xh).sum(ax, dtype=f32)
    dx = sf * ((g - dbeta / R) - xh * (dgamma / R))
    return y, dx.astype(f32), dgamma, dbeta


# ----------------------------------------------------------------------------- the predictor
def predictor(W, feats, num_classes, training=True, d_boxes=None, d_classes=None):
    """W {name: array}, feats [p3 ..] NHWC -> (encoded_boxes [B,N,4], class_predictions [B,N,C]) in float64; with the upstream
    gradients d_boxes / d_classes also (grads {name: array}, [d p3 ..])."""
    n = len(feats)
    B = feats[0].shape[0]
    W = {k: np.asarray(v, np.float64) for k, v in W.items()}
    outs, tapes = {}, {}
    for net, last, width in (("box_net", "encoded_boxes", 4), ("class_net", "logits", num_classes)):
        x = [f.astype(np.float64) for f in feats]
        tape = []
        for i in range(4):
            k = W["%s/conv3x3_%d/kernel" % (net, i)]
            c = [conv3x3(v, k) for v in x]
            y = []
            for l in range(n):
                s = "%s/batch_norm_%d_for_level_%d" % (net, i, 3 + l)
                if training:
                    y.append(bn_relu_forward(c[l], W[s + "/gamma"], W[s + "/beta"])[0])
                else:
                    sf = W[s + "/gamma"] / np.sqrt(W[s + "/moving_variance"] + EPS)
                    y.append(np.maximum((c[l] - W[s + "/moving_mean"]) * sf + W[s + "/beta"], 0.0))
            tape.append((x, c))
            x = y
        o = [conv3x3(v, W["%s/%s/kernel" % (net, last)], W["%s/%s/bias" % (net, last)]) for v in x]
        tapes[net] = (tape, x, [v.shape for v in o])
        outs[net] = np.concatenate([v.reshape(B, -1, width) for v in o], axis=1)
    if d_boxes is None:
        return outs["box_net"], outs["class_net"]
    grads, dfeats = {}, [np.zeros(f.shape, np.float64) for f in feats]
    for net, last, d in (("box_net", "encoded_boxes", d_boxes), ("class_net", "logits", d_classes)):
        tape, xlast, shapes = tapes[net]
        d = d.astype(np.float64)
        dys, at = [], 0
        for s in shapes:
            cnt = s[1] * s[2] * s[3] // d.shape[2]
            dys.append(d[:, at:at + cnt].reshape(s))
            at += cnt
        dxs, dw, db = conv3x3_grads(xlast, W["%s/%s/kernel" % (net, last)], dys)
        grads["%s/%s/kernel" % (net, last)], grads["%s/%s/bias" % (net, last)] = dw, db
        for i in range(3, -1, -1):
            x, c = tape[i]
            dc = []
            for l in range(n):
                s = "%s/batch_norm_%d_for_level_%d" % (net, i, 3 + l)
                dx, dg, dbt = bn_relu_backward(c[l], W[s + "/gamma"], W[s + "/beta"], dxs[l])
                grads[s + "/gamma"], grads[s + "/beta"] = dg, dbt
                dc.append(dx)
            dxs, dw, _ = conv3x3_grads(x, W["%s/conv3x3_%d/kernel" % (net, i)], dc)
            grads["%s/conv3x3_%d/kernel" % (net, i)] = dw
        for l in range(n):
            dfeats[l] += dxs[l]
    return grads, dfeats


# ----------------------------------------------------------------------------- the loss, for whole-graph runs in one precision
def torch_loss(class_predictions, encoded_boxes, anchors, boxes, labels, num, gamma=2.0, alpha=0.25, pos=0.5, neg=0.5):
    """localization_loss + classification_loss (losses.py, ssd.py:71-133) in torch ops of the dtype of its inputs, differentiable;
    the matching and the targets (discrete, independent of the predictions) come from loss_ref.training_targets.  1 - sigmoid(x)
    as sigmoid(-x) and -log p_t as softplus, the formulation of test_loss_grad_host's float64 restatement."""
    import torch
    from helpers import loss_ref
    x, codes = class_predictions, encoded_boxes
    B, N, C = x.shape
    t = [loss_ref.training_targets(anchors, boxes[b][:int(num[b])], labels[b][:int(num[b])], pos, neg) for b in range(B)]
    reg = torch.tensor(np.stack([v[0] for v in t]).astype(np.float64), dtype=x.dtype)
    cls = torch.tensor(np.stack([v[1] for v in t]).astype(np.int64))
    m = torch.tensor(np.stack([v[2] for v in t]).astype(np.int64))
    z = torch.nn.functional.one_hot(cls, C + 1)[:, :, 1:].bool()
    a, oma = float(f32(alpha)), float(f32(1.0 - alpha))
    sp = lambda v: torch.nn.functional.softplus(v, beta=1.0, threshold=1000.0)
    fl = torch.where(z, a * torch.sigmoid(-x) ** gamma * sp(-x), oma * torch.sigmoid(x) ** gamma * sp(x))
    cls_loss = (fl.sum(2) * (m >= -1).to(x.dtype)).sum()
    diff = codes - reg
    ad = diff.abs()
    sl = torch.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5)
    loc_loss = (sl.sum(2) * (m >= 0).to(x.dtype)).sum()
    norm = float(max(f32(int((m >= 0).sum())), f32(1)))
    return loc_loss / norm + cls_loss / norm, int((m >= 0).sum(1).min())
