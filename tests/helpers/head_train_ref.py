"""Float64 numpy restatement of the TRAIN head (include/ssd_hip.h, "the TRAIN head"): the training-mode batch norm + ReLU with its
gradients and the whole RetinaNetBoxPredictor (box_predictor.py:34-155) forward and backward over helpers.train_ops_ref's
convolution (re-exported here: the head is its k = 3, stride 1 case); plus the float32 restatement of the batch norm in the
header's operation order."""
import numpy as np

from helpers.train_ops_ref import conv, conv_grads, integer_premise, rotated_transposed, rows_per_slice, wgrad_bound   # noqa: F401

EPS = 1e-3
MOMENTUM = 0.993
f32 = np.float32


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
            c = [conv(v, k) for v in x]
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
        o = [conv(v, W["%s/%s/kernel" % (net, last)], bias=W["%s/%s/bias" % (net, last)]) for v in x]
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
        dxs, dw, db = conv_grads(xlast, W["%s/%s/kernel" % (net, last)], dys)
        grads["%s/%s/kernel" % (net, last)], grads["%s/%s/bias" % (net, last)] = dw, db
        for i in range(3, -1, -1):
            x, c = tape[i]
            dc = []
            for l in range(n):
                s = "%s/batch_norm_%d_for_level_%d" % (net, i, 3 + l)
                dx, dg, dbt = bn_relu_backward(c[l], W[s + "/gamma"], W[s + "/beta"], dxs[l])
                grads[s + "/gamma"], grads[s + "/beta"] = dg, dbt
                dc.append(dx)
            dxs, dw, _ = conv_grads(x, W["%s/conv3x3_%d/kernel" % (net, i)], dc)
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


# ----------------------------------------------------------------------------- the header's arithmetic, for the edge tests
def al256(v):
    return (v + 255) // 256 * 256


def slab_plan(rows, C):
    """include/ssd_hip.h's slab formula for a batch-norm call with these per-level rows -> (rpp, slab_rows, total slabs)."""
    G = (min(C, 1024) + 3) // 4
    rpp = 256 // G
    sr = max(8 * rpp, -(-sum(rows) // 1024))
    sr = -(-sr // rpp) * rpp
    return rpp, sr, sum(-(-r // sr) for r in rows)


def bn_gate_f32(x, gamma, beta, mean, var, dy, eps=EPS):
    """The backward's float32 operands as the header forms them: g = (t * sf + beta > 0 ? dy : 0) and xhat = t * invstd, with
    t = x - mean, sf = gamma * invstd, one float32 operation at a time."""
    x, gamma, beta, mean = (v.astype(f32) for v in (x, gamma, beta, mean))
    invstd = invstd_f32(var, eps)
    t = x - mean
    ypre = t * (gamma * invstd) + beta
    return np.where(ypre > 0, dy.astype(f32), f32(0)), t * invstd


def double_sum_bound(terms):
    """terms float64 [rows, C] -> (want, tol): `want` is the EXACT column sum (math.fsum) rounded once to float32, and
    |got - want| <= tol holds for the float32 rounding `got` of ANY order of double-precision summation of the same terms.
    Derivation: n terms added in double in any order give S' with |S' - S| <= gamma_(n-1) * sum|t|, gamma_k = k u / (1 - k u),
    u = 2^-53 (Higham, Accuracy and Stability, eq. 4.4), and gamma_(n-1) <= n u while n < 2^26: E = n * 2^-53 * sum|t|.  Rounding
    to float32 is monotonic, so got = fl(S') lies between fl(S - E) and fl(S + E): at most E plus half a float32 ulp on either
    side away from fl(S), the ulps taken at |S| + E (the spacing of the larger neighbour): tol = E + ulp32(|S| + E).  A column
    that contains a non-finite term gives want = nan, tol = nan: compare it separately."""
    import math
    terms = np.asarray(terms, np.float64)
    n = terms.shape[0]
    assert n < 2 ** 26
    finite = np.isfinite(terms).all(0)
    exact = np.array([math.fsum(terms[:, c].tolist()) if finite[c] else np.nan for c in range(terms.shape[1])])
    E = n * 2.0 ** -53 * np.abs(terms).sum(0)
    with np.errstate(invalid="ignore"):
        tol = E + np.spacing((np.abs(exact) + E).astype(f32)).astype(np.float64)
    return exact.astype(f32), tol


def offset_variance_bound(offset, var):
    """Relative distance allowed between the header's variance (float64 around the float32 mean m32, rounded once) and the true
    float64 variance: the sum around m32 is var + (m32 - m)^2 with |m32 - m| <= ulp32(offset) / 2, i.e. (ulp / 2)^2 / var relative,
    plus 2^-24 for the final rounding; 2 ulp^2 / var covers both wherever ulp^2 / var >= 2^-24 (asserted)."""
    ulp = float(np.spacing(f32(offset)))
    assert ulp * ulp / var >= 2.0 ** -24
    return 2.0 * ulp * ulp / var


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_head_train_edges.py
PYRAMID = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]
EIGHT = [(9, 11), (8, 7), (6, 5), (5, 5), (4, 3), (3, 2), (2, 1), (1, 1)]
# name: (B, level sizes, Cin, Cout).  Widths: Cout = 6 * classes for 1, 3 and 20 classes (6 and 18 are no multiples of 4: the
# 32-wide tile with element-wise dy loads); Cin that is no multiple of 32 / 128, Cin above 256 (three ci tiles, the last with 8
# channels), Cout just past a tile edge.  Geometry: B = 1 and 3, thin levels, fewer rows than one K-step, eight levels, a level
# that is a whole number of slices beside one that is one row more (B = 1: 16 * 32 = 512 and 27 * 19 = 513 rows, slices of 256).
CONV_CASES = {
    "256-6": (2, PYRAMID, 256, 6), "256-18": (2, PYRAMID, 256, 18), "256-120": (2, PYRAMID, 256, 120),
    "24-24": (2, PYRAMID, 24, 24), "72-33": (2, PYRAMID, 72, 33), "136-129": (2, PYRAMID, 136, 129),
    "264-132": (2, PYRAMID, 264, 132), "8-1": (2, PYRAMID, 8, 1),
    "B1": (1, PYRAMID, 64, 40), "B3": (3, PYRAMID, 256, 18),
    "thin": (2, [(7, 9), (1, 37), (29, 1), (1, 1)], 64, 40),
    "six-rows": (1, [(3, 2)], 24, 18),
    "eight-levels": (2, EIGHT, 64, 40),
    "slice-edge": (1, [(16, 32), (27, 19)], 64, 40),
}


def conv_case_data(name, integers):
    """-> (B, sizes, xs, w, bias, dys) of a CONV_CASES entry: small integers (|x|, |dy| <= 3, |w| <= 2) or random normal data."""
    import zlib
    B, sizes, Cin, Cout = CONV_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + (1 if integers else 0))
    if integers:
        xs = [rng.integers(-3, 4, (B, h, w, Cin)).astype(f32) for h, w in sizes]
        dys = [rng.integers(-3, 4, (B, h, w, Cout)).astype(f32) for h, w in sizes]
        w = rng.integers(-2, 3, (3, 3, Cin, Cout)).astype(f32)
        bias = rng.integers(-4, 5, Cout).astype(f32)
    else:
        xs = [rng.normal(0, 1, (B, h, w, Cin)).astype(f32) for h, w in sizes]
        dys = [rng.normal(0, 1, (B, h, w, Cout)).astype(f32) for h, w in sizes]
        w = rng.normal(0, 0.05, (3, 3, Cin, Cout)).astype(f32)
        bias = rng.normal(0, 0.1, Cout).astype(f32)
    return B, sizes, xs, w, bias, dys


# ----------------------------------------------------------------------------- the predictor's whole-graph inputs
def groundtruth(ssd, batch, seed, height=128, width=128):
    """Anchors of a height x width image and, per image, one box on a jittered anchor of EVERY pyramid level (unclipped: the
    anchors of p6 and p7 can be larger than the image), so that both nets receive a gradient at every level."""
    g = ssd.AnchorGenerator()
    anchors = g(height, width)
    per_level = list(g.num_anchors_per_feature_map)
    rng = np.random.default_rng(seed)
    boxes = np.zeros((batch, len(per_level), 4), f32)
    for b in range(batch):
        at = 0
        for l, n in enumerate(per_level):
            a = anchors[at + rng.integers(0, n)]
            boxes[b, l] = a + rng.normal(0, 0.02, 4) * (a[2] - a[0])
            at += n
    return anchors, boxes, rng.integers(0, 80, boxes.shape[:2]).astype(np.int32), np.full(batch, len(per_level), np.int32)


LARGE_SIZES = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]          # the pyramid of a 320 x 448 image


def large_predictor_input(ssd, params):
    """The second whole-graph input: B = 3, random normal p3 .. p7 of a 320 x 448 image (256 channels; not from an engine), its
    anchors, one jittered ground-truth box per level.  -> (W, feats, anchors, boxes, labels, num)."""
    W = ssd.synthetic_weights(params, seed=21, logits_bias=-4.0)
    rng = np.random.default_rng(22)
    feats = [rng.normal(0, 1, (3, h, w, 256)).astype(f32) for h, w in LARGE_SIZES]
    return (W, feats) + groundtruth(ssd, 3, 23, 320, 448)


def predictor_references(W, feats, anchors, boxes, labels, num, num_classes=80):
    """The reference and the yardstick of the predictor's training-mode test, on the CPU.  Reference: the float64 restatement
    with the loss's gradient by float64 torch autograd at its float64 outputs.  Yardstick: the same graph, loss included, in
    float32 CPU torch ops, one backward.  -> (least matches per image, [(name, float32 value, float64 value)]) over the two
    outputs, the gradient of every variable and of every feature map."""
    from test_head_train_host import _torch_predictor
    import torch
    head = {k: v for k, v in W.items() if k.startswith(("box_net/", "class_net/"))}
    eb64, cp64 = predictor(head, feats, num_classes)
    tcp, teb = torch.tensor(cp64, requires_grad=True), torch.tensor(eb64, requires_grad=True)
    total64, least = torch_loss(tcp, teb, anchors, boxes, labels, num)
    total64.backward()
    g64, df64 = predictor(head, feats, num_classes, d_boxes=teb.grad.numpy(), d_classes=tcp.grad.numpy())
    (tb, tc), T, P = _torch_predictor(head, feats, num_classes, dtype=torch.float32)
    total32, _ = torch_loss(tc, tb, anchors, boxes, labels, num)
    assert total32.dtype == torch.float32
    total32.backward()
    rows = [("encoded_boxes", tb.detach().numpy(), eb64), ("class_predictions", tc.detach().numpy(), cp64)]
    rows += [("d " + name, T[name].grad.numpy(), g64[name]) for name in g64]
    rows += [("d p%d" % (3 + l), P[l].grad.numpy(), df64[l]) for l in range(len(feats))]
    return least, rows


def rel(a, r):
    """max |a - r| / max |r|: the predictor tests' norm-wise figure."""
    return float(np.abs(np.asarray(a, np.float64) - r).max() / np.abs(r).max())
