"""The matching and loss kernels of loss.hip where a kernel goes wrong and a numpy restatement cannot: arg-max ties by
position (threads, lanes, waves, blocks, gt tiles), forced-match collisions, gt that overlap nothing, IoUs on the
thresholds, edge sizes and a grid fuzz, against the exact integer reference (tests/helpers/match_exact.py) on hand-built
anchor tables (tests/helpers/loss_edge_cases.py); and the focal / smooth-L1 branches no other forward test executes
(gamma != 2, unaligned logits, logits where exp(-|x|) underflows, |code - target| == 1) against loss_ref / loss_grad_ref."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import loss_edge_cases as cases
from helpers import loss_grad_ref, loss_ref, match_exact

pytestmark = pytest.mark.gpu

FLT_MIN = np.float32(1.17549435e-38)


def _ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_case(ssd, cuda, case):
    """matches / cls_targets identical to the exact reference, reg_targets against loss_ref.encode (ty, tx bit-equal, th, tw
    within 1 ulp), a second launch bit-equal; returns the reference matches [setting][image]."""
    anchors, boxes, labels, num = case["anchors"], case["boxes"], case["labels"], case["num"]
    a_dev = cuda.from_numpy(anchors).cuda()
    B, G, N = len(num), boxes.shape[1], len(anchors)
    want = [match_exact.training_targets_multi(anchors, boxes[b, :min(max(int(num[b]), 0), G)], labels[b], case["settings"])
            for b in range(B)]
    out = []
    for k, (pos, neg) in enumerate(case["settings"]):
        got = [t.cpu().numpy() for t in ssd.get_training_targets(a_dev, boxes, labels, num, pos, neg)]
        again = [t.cpu().numpy() for t in ssd.get_training_targets(a_dev, boxes, labels, num, pos, neg)]
        for x, y in zip(got, again):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (case["name"], "second launch")
        reg, cls, m = got
        assert reg.shape == (B, N, 4) and cls.shape == (B, N) and m.shape == (B, N)
        for b in range(B):
            w_cls, w_m = want[b][k]
            bad = np.flatnonzero(m[b] != w_m)
            assert bad.size == 0, (case["name"], "image", b, (pos, neg), "anchors", bad[:8], "got", m[b][bad[:8]], "want", w_m[bad[:8]])
            assert np.array_equal(cls[b], w_cls), (case["name"], b, (pos, neg))
            w_reg = np.zeros((N, 4), np.float32)
            hit = w_m >= 0
            if hit.any():
                w_reg[hit] = loss_ref.encode(boxes[b][w_m[hit]], anchors[hit])
            assert np.array_equal(reg[b][:, :2], w_reg[:, :2]), (case["name"], b)
            assert _ulp_diff(reg[b][:, 2:], w_reg[:, 2:]).max() <= 1, (case["name"], b)
        out.append([want[b][k][1] for b in range(B)])
    return out


@pytest.mark.parametrize("make", [cases.anchor_ties, cases.gt_ties, cases.collisions, cases.zero_overlap, cases.thresholds],
                         ids=["anchor_ties", "gt_ties", "collisions", "zero_overlap", "thresholds"])
def test_hand_built_matching(ssd, cuda, make):
    for case in make():
        _check_case(ssd, cuda, case)


@pytest.mark.parametrize("index", range(len(cases.SIZES_N) + len(cases.SIZES_G) + 2))
def test_sizes(ssd, cuda, index):
    _check_case(ssd, cuda, cases.sizes()[index])


def test_more_than_4096_gt_is_refused(ssd, cuda):
    anchors = cuda.zeros((8, 4), device="cuda")
    boxes, labels = np.zeros((1, 4097, 4), np.float32), np.zeros((1, 4097), np.int32)
    with pytest.raises(ssd.SsdError, match="4096"):
        ssd.get_training_targets(anchors, boxes, labels, [4097])
    with pytest.raises(ssd.SsdError, match="4096"):
        ssd.ssd_loss(cuda.zeros((1, 8, 2), device="cuda"), cuda.zeros((1, 8, 4), device="cuda"), anchors,
                     {"boxes": boxes, "labels": labels, "num_boxes": [4097]})


def _level_counts(m, levels):
    edges = np.cumsum([0] + list(levels))
    return [float((m[edges[k]:edges[k + 1]] >= 0).sum()) for k in range(len(levels))]


@pytest.mark.parametrize("seed", range(cases.FUZZ_SEEDS))
def test_grid_fuzz(ssd, cuda, seed):
    """Integer corners in [0, 12]: thousands of equal IoUs and many collisions per table (counted in
    test_match_exact_host.py).  No case is skipped or filtered here."""
    case = cases.fuzz_case(seed)
    want = _check_case(ssd, cuda, case)
    B, N = len(case["num"]), len(case["anchors"])
    dev = [cuda.zeros((B, N, 1), device="cuda"), cuda.zeros((B, N, 4), device="cuda"), cuda.from_numpy(case["anchors"]).cuda()]
    gt = {"boxes": case["boxes"], "labels": case["labels"] % 1, "num_boxes": case["num"]}
    for k, (pos, neg) in enumerate(case["settings"]):
        _, per = ssd.ssd_loss(*dev, gt, anchors_per_level=case["levels"], positives_threshold=pos, negatives_threshold=neg)
        per = per.cpu().numpy()
        assert per.shape == (B, 3 + len(case["levels"]))
        for b in range(B):
            assert per[b, 2] == float((want[k][b] >= 0).sum()), (seed, b, pos, neg)
            assert per[b, 3:].tolist() == _level_counts(want[k][b], case["levels"]), (seed, b, pos, neg)


def test_level_end_at_a_levels_first_and_last_anchor(ssd, cuda):
    """Every anchor matched (each gt equals one anchor, forced) and levels of 1, 0, 63, 1, 64, 0, 1, N - 130 anchors: a
    level's first and last anchor on both sides of a block of 64."""
    N = 300
    anchors = np.array([[y, x, y + 1, x + 1] for y in range(20) for x in range(15)], np.float32)
    levels = (1, 0, 63, 1, 64, 0, 1, N - 130)
    boxes, labels = anchors[None].copy(), np.zeros((1, N), np.int32)
    _, per = ssd.ssd_loss(cuda.zeros((1, N, 1), device="cuda"), cuda.zeros((1, N, 4), device="cuda"), cuda.from_numpy(anchors).cuda(),
                          {"boxes": boxes, "labels": labels, "num_boxes": [N]}, anchors_per_level=levels)
    assert per.cpu().numpy()[0, 2:].tolist() == [float(N)] + [float(v) for v in levels]
    assert match_exact.training_targets(anchors, boxes[0], labels[0])[1].tolist() == list(range(N))


def test_every_combination_of_optional_outputs(ssd, cuda):
    """The ABI makes each output optional: every None / non-None combination of ssd_training_targets' three and ssd_loss's
    four gives the bits of the call with all of them, and leaves nothing else written."""
    case = cases.zero_overlap()[0]
    anchors, boxes, labels, num = case["anchors"], case["boxes"], case["labels"] % 3, case["num"]
    B, G, N, C = len(num), boxes.shape[1], len(anchors), 3
    L = ssd.lib()
    rng = np.random.default_rng(5)
    a, bx, lb, nm = (cuda.from_numpy(np.ascontiguousarray(x)).cuda() for x in (anchors, boxes, labels, num))
    lg = cuda.from_numpy(rng.normal(-2, 2, (B, N, C)).astype(np.float32)).cuda()
    cd = cuda.from_numpy(rng.normal(0, 1.5, (B, N, 4)).astype(np.float32)).cuda()
    nbytes = L.ssd_loss_workspace_bytes(B, N, G)
    ws = cuda.empty((nbytes,), dtype=cuda.uint8, device="cuda")
    cfg = ssd.ssd._loss_config(0.5, 0.25, 1.5, 0.3, (40, 50))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    full_t = ssd.get_training_targets(a, boxes, labels, num, 0.5, 0.25)
    full_l = ssd.ssd_loss(lg, cd, a, {"boxes": boxes, "labels": labels, "num_boxes": num}, 1.5, 0.3, (40, 50), True, 0.5, 0.25)
    full_l = (full_l[1], full_l[0], full_l[2], full_l[3])                   # the ABI's order: per_image, losses, cls, loc
    for use in itertools.product([False, True], repeat=3):
        outs = [cuda.full_like(t, -7) if u else None for t, u in zip(full_t, use)]
        assert L.ssd_training_targets(p(a), N, p(bx), p(lb), p(nm), B, G, ctypes.byref(cfg), p(outs[0]), p(outs[1]), p(outs[2]),
                                      p(ws), nbytes, None) == 0, L.ssd_last_error()
        cuda.cuda.synchronize()
        for o, f in zip(outs, full_t):
            assert o is None or cuda.equal(o, f), use
    for use in itertools.product([False, True], repeat=4):
        outs = [cuda.full_like(t, -7) if u else None for t, u in zip(full_l, use)]
        assert L.ssd_loss(p(lg), p(cd), p(a), B, N, C, p(bx), p(lb), p(nm), G, ctypes.byref(cfg), p(outs[0]), p(outs[1]), p(outs[2]),
                          p(outs[3]), p(ws), nbytes, None) == 0, L.ssd_last_error()
        cuda.cuda.synchronize()
        for o, f in zip(outs, full_l):
            assert o is None or cuda.equal(o, f), use


# ----------------------------------------------------------------------------- loss values on the untested branches
GAMMAS = (0.0, 0.5, 1.0, 1.5, 3.0, 5.0)
ALPHAS = (0.25, 0.5, 0.9)
COUNTS = [5, 0, 40]


def _assert_grad_close(got, want64, what):
    """test_gpu_loss_grad.py's rule: within 1 ulp of the float64 value rounded once, or both below FLT_MIN; zeros exact."""
    want = want64.astype(np.float32)
    assert not np.isnan(got).any(), (what, np.argwhere(np.isnan(got))[:5])
    zero = want64 == 0
    assert np.array_equal(got[zero], want[zero]), what
    ok = (_ulp_diff(got, want) <= 1) | ((np.abs(got) < FLT_MIN) & (np.abs(want) < FLT_MIN))
    assert ok.all(), (what, np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])


def _check_values(ssd, cuda, anchors, levels, logits, codes, boxes, labels, num, gamma, alpha, what, f64=True):
    """Forward against the restatement (per-anchor values rtol 1e-6, match counts exact, scalars 1e-6) and float64 (1e-5);
    the gradient against loss_grad_ref at its 1-ulp rule."""
    a = cuda.from_numpy(anchors).cuda()
    lg, cd = cuda.from_numpy(logits).cuda(), cuda.from_numpy(codes).cuda()
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    losses, per, cl, ll = (t.cpu().numpy() for t in ssd.ssd_loss(lg, cd, a, gt, gamma, alpha, levels, True))
    with np.errstate(over="ignore"):
        r_losses, r_per, r_cl, r_ll = loss_ref.batch_losses(logits, codes, anchors, boxes, labels, num, gamma=gamma, alpha=alpha)
        w64 = loss_ref.losses_f64(logits, codes, anchors, boxes, labels, num, gamma=gamma, alpha=alpha)
    print(what, "losses", losses, "restatement", r_losses, "float64", w64)
    np.testing.assert_allclose(cl, r_cl, rtol=1e-6, atol=0, err_msg=str(what))
    np.testing.assert_allclose(ll, r_ll, rtol=1e-6, atol=0, err_msg=str(what))
    np.testing.assert_allclose(per[:, :2], r_per[:, :2], rtol=1e-6, err_msg=str(what))
    assert np.array_equal(per[:, 2], r_per[:, 2]), what
    for b in range(len(num)):
        m = loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]])[2]
        assert per[b, 3:].tolist() == _level_counts(m, levels), what
    np.testing.assert_allclose(losses, r_losses, rtol=1e-6, err_msg=str(what))
    if f64:
        np.testing.assert_allclose(losses, w64, rtol=1e-5, err_msg=str(what))
    reg, cls, m = ssd.get_training_targets(a, boxes, labels, num)
    d_l, d_c = ssd.ssd_loss_backward(lg, cd, reg, cls, m, cuda.from_numpy(per).cuda(), gamma, alpha, grad_losses=(1.0, 2.0))
    w_l, w_c = loss_grad_ref.batch_grads(logits, codes, anchors, boxes, labels, num, gamma, alpha, (1.0, 2.0))
    _assert_grad_close(d_l.cpu().numpy(), w_l, (what, "d_logits"))
    _assert_grad_close(d_c.cpu().numpy(), w_c, (what, "d_codes"))
    return losses, per, cl, ll


def _small_image(ssd):
    g = ssd.AnchorGenerator()
    anchors = g(128, 128)
    return anchors, tuple(g.num_anchors_per_feature_map)


@pytest.mark.parametrize("C", [1, 3, 4, 80])
def test_focal_pow_branch(ssd, cuda, C):
    """gamma != 2 takes focal_term's pow branch, which no other forward test executes."""
    anchors, levels = _small_image(ssd)
    logits, codes, boxes, labels, num = cases.value_inputs(anchors, C, COUNTS, seed=30 + C)
    for gamma in GAMMAS:
        for alpha in ALPHAS:
            _check_values(ssd, cuda, anchors, levels, logits, codes, boxes, labels, num, gamma, alpha, (C, gamma, alpha))


@pytest.mark.parametrize("C", [80, 4])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_unaligned_logits_take_the_scalar_path_with_the_same_bits(ssd, cuda, C, gamma):
    """C % 4 == 0 with the logits 1, 2 and 3 floats past a 16-byte boundary (the wrapper passes data_ptr() through)."""
    anchors, levels = _small_image(ssd)
    logits, codes, boxes, labels, num = cases.value_inputs(anchors, C, COUNTS, seed=40 + C)
    B, N = logits.shape[:2]
    a, cd = cuda.from_numpy(anchors).cuda(), cuda.from_numpy(codes).cuda()
    gt = {"boxes": boxes, "labels": labels, "num_boxes": num}
    buf = cuda.zeros((B * N * C + 4,), device="cuda")
    outs = []
    for offset in range(4):
        lg = buf[offset:offset + B * N * C].view(B, N, C)
        lg.copy_(cuda.from_numpy(logits))
        assert lg.data_ptr() % 16 == 4 * offset and lg.is_contiguous()
        outs.append([t.cpu().numpy() for t in ssd.ssd_loss(lg, cd, a, gt, gamma, 0.25, levels, True)])
    for offset in (1, 2, 3):
        for x, y in zip(outs[0], outs[offset]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (C, gamma, offset)
    r_cl = loss_ref.batch_losses(logits, codes, anchors, boxes, labels, num, gamma=gamma)[2]
    np.testing.assert_allclose(outs[0][2], r_cl, rtol=1e-6, atol=0)


def _planted(ssd, anchors, C, values, seed):
    logits, codes, boxes, labels, num = cases.value_inputs(anchors, C, COUNTS, seed=seed)
    tg = [loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]]) for b in range(len(num))]
    reg, cls, m = (np.stack([t[k] for t in tg]) for k in range(3))
    assert cases.plant_logits(logits, cls, m, values) > 0
    mask = cases.plant_codes(codes, reg, m)
    assert mask.sum() >= 2 * cases.EQUAL_GT                                  # every delta on some matched anchor
    return logits, codes, boxes, labels, num, mask


@pytest.mark.parametrize("C", [80, 3])
@pytest.mark.parametrize("gamma", [2.0, 0.0, 0.5, 1.0, 1.5, 3.0])
@pytest.mark.parametrize("values", [cases.MODERATE, cases.PLANTED], ids=["moderate", "extreme"])
def test_planted_logits_and_codes(ssd, cuda, values, gamma, C):
    """Logits at 0, +-1e-30, +-16.6, +-17.4 (exp(-|x|) around fp32 epsilon), +-88, +-104 (the underflow of a float), +-720
    (exp(-|x|) denormal in double) and +-1e4 (0 in double: the sigmoid is exactly 0 or 1, q == 0 in the gradient) on target and
    background classes; codes with code - target exactly +-1, +-(1 - 2^-24), +-(1 + 2^-23) and 0 on matched anchors.
    The restatement alone meets the float64 bound on these inputs (test_match_exact_host.py), so nothing is kept out of
    the float64 comparison.  gamma < 1: the first term of the gradient is gamma * q^gamma * (+-(1 - q)) * nlp in float64,
    0 at q == 0 for every gamma > 0 and finite on a denormal q; kernel and helper once formed q^(gamma-1) and gave NaN at
    gamma == 0, |x| = 720 (0 * inf).  Both now evaluate the folded form."""
    anchors, levels = _small_image(ssd)
    logits, codes, boxes, labels, num, mask = _planted(ssd, anchors, C, values, seed=50 + C)
    _l, _p, _cl, ll = _check_values(ssd, cuda, anchors, levels, logits, codes, boxes, labels, num, gamma, 0.25,
                                    (C, gamma, values[-1]))
    # the planted codes, spelled out: the GPU's targets there are exactly 0, so |code - target| is the planted value
    reg, _cls, m = (t.cpu().numpy() for t in ssd.get_training_targets(cuda.from_numpy(anchors).cuda(), boxes, labels, num))
    assert (reg[mask] == 0).all() and (m[mask] >= 0).all()
    d = np.abs(codes[mask])
    assert (d == 1).any() and (d == np.float32(1 - 2.0 ** -24)).any() and (d == np.float32(1 + 2.0 ** -23)).any() and (d == 0).any()
    want = np.where(d < 1, np.float32(0.5) * (d * d), d - np.float32(0.5)).astype(np.float64).sum(axis=1).astype(np.float32)
    assert np.array_equal(ll[mask], want)
