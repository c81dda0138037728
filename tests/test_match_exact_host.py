"""The exact matching reference (tests/helpers/match_exact.py) pinned before the GPU sees it (no GPU): it agrees with the
float32 restatement (tests/helpers/loss_ref.py) on every input generator of tests/helpers/loss_edge_cases.py, both
reproduce the hand-worked cases of test_loss_host.py on integer coordinates, the fuzz seeds contain the ties and
collisions they are meant to, and the restatement's batch scalars stay within 1e-5 of float64 on the planted logits."""
import numpy as np
import pytest

from helpers import loss_edge_cases as cases
from helpers import loss_ref, match_exact


def _both(case, stats=None):
    """Every image and threshold setting of a case through both references; returns the exact matches [setting][image]."""
    out = [[] for _ in case["settings"]]
    for b in range(len(case["num"])):
        n = min(max(int(case["num"][b]), 0), case["boxes"].shape[1])
        gt, lb = case["boxes"][b, :n], case["labels"][b, :n]
        st = {} if stats is not None else None
        res = match_exact.training_targets_multi(case["anchors"], gt, lb, case["settings"], stats=st)
        if stats is not None:
            stats.append(st)
        for k, ((pos, neg), (cls, m)) in enumerate(zip(case["settings"], res)):
            _reg, r_cls, r_m = loss_ref.training_targets(case["anchors"], gt, lb, pos, neg)
            assert np.array_equal(m, r_m), (case["name"], b, pos, neg, np.flatnonzero(m != r_m)[:10])
            assert np.array_equal(cls, r_cls), (case["name"], b, pos, neg)
            out[k].append(m)
    return out


@pytest.mark.parametrize("make", [cases.anchor_ties, cases.gt_ties, cases.collisions, cases.zero_overlap, cases.thresholds,
                                  lambda: cases.sizes(small=True)],
                         ids=["anchor_ties", "gt_ties", "collisions", "zero_overlap", "thresholds", "sizes"])
def test_exact_reference_agrees_with_the_restatement(make):
    for case in make():
        _both(case)


def test_hand_built_cases_hold_what_they_claim():
    """The answers the generators' docstrings promise, from the exact reference."""
    m = _both(cases.anchor_ties()[0])
    for c in range(2 * len(cases.ANCHOR_PAIRS)):
        i, j = cases.ANCHOR_PAIRS[c % len(cases.ANCHOR_PAIRS)]
        b, row = c // 4, cases.GT_ROWS[c % 4]
        if c < len(cases.ANCHOR_PAIRS):                                           # IoU 1: both matched
            assert m[0][b][i] == row and m[0][b][j] == row
        else:                                                                     # IoU 1/3: the lower index alone, forced
            assert (m[0][b][i], m[0][b][j]) == (row, -1) and (m[1][b][i], m[1][b][j]) == (row, -2)
    case = cases.gt_ties()[0]
    m = _both(case)
    for k, (g, _h) in enumerate(cases.GT_PAIRS):
        assert m[0][0][17 * k + 3] == g and m[0][0][17 * k + 70] == -1 and m[1][0][17 * k + 70] == -2
    m = _both(cases.collisions()[0])[0][0]
    v = 0
    for k in (2, 3, 5):
        for kind in ("first_passes", "first_fails", "all_fail"):
            x_row = 5 + v if v % 2 else 400 + v
            assert m[13 * v + 1] == (x_row if kind == "all_fail" else 20 + 7 * v), (k, kind)
            assert m[13 * v + 200] == x_row
            v += 1
    m = _both(cases.zero_overlap()[0])[0]
    assert (m[0] == -1).all() and m[1][0] == 4 and m[2][0] == -1 and m[2][1] == 3 and m[3][0] == 2
    assert m[4][0] == 0 and m[4][2] == 7 and m[4][10] == -1 and m[4][11] == -1
    m = _both(cases.thresholds()[0])
    probes = [2 * y for y in range(len(cases.PLAIN_STRIPS))] + [2 * len(cases.PLAIN_STRIPS) + y for y in range(len(cases.FORCED_STRIPS))]
    assert [int(m[0][0][p]) for p in probes] == [0, -1, -1, -1, 4, -1, 6, -1, -1, 9, 10, -1]
    assert [int(m[1][0][p]) for p in probes] == [0, -2, -2, -1, 4, -2, 6, -1, -1, 9, 10, -1]
    assert np.float32(3) / np.float32(30) == np.float32(0.1) and np.float32(1) / np.float32(10) == np.float32(0.1)
    by_name = {c["name"]: c for c in cases.sizes(small=True)}
    m = _both(by_name["gt_num clamped"])[0]
    assert (m[0] == -1).all() and (m[1] == -1).all() and (m[2] >= 0).sum() >= 20 and (m[3] >= 0).sum() >= 20
    case = by_name["gt_num partial"]
    m = _both(case)[0]
    assert m[0].max() < 7 and m[1].max() < 13
    full = match_exact.training_targets(case["anchors"], case["boxes"][0], case["labels"][0])[1]
    assert full.max() >= 7                                                        # the rows beyond the count would win


def test_both_reproduce_the_hand_worked_cases_on_integer_coordinates():
    """test_loss_host.py's five restatement cases with the coordinates scaled to integers (x 20, the last x 100 / 3.125)."""
    def both(anchors, gt, labels, **kw):
        cls, m = match_exact.training_targets(anchors, gt, labels, **kw)
        _reg, r_cls, r_m = loss_ref.training_targets(np.asarray(anchors, np.float32), np.asarray(gt, np.float32).reshape(-1, 4),
                                                      labels, **kw)
        assert np.array_equal(m, r_m) and np.array_equal(cls, r_cls)
        return m.tolist(), cls.tolist()
    # a tie takes the first gt
    assert both([[0, 0, 20, 20], [0, 0, 10, 10]], [[0, 0, 20, 20], [0, 0, 20, 20]], [7, 3]) == ([0, -1], [8, 0])
    # a forced collision with a masked first row: IoU 1/400 (masked) and 100/400, both pick anchor 0 -> gt 0
    assert both([[0, 0, 20, 20], [25, 25, 30, 30]], [[0, 0, 1, 1], [0, 0, 10, 10]], [4, 9]) == ([0, -1], [5, 0])
    # a gt whose IoUs are all 0 is never forced
    assert both([[0, 0, 10, 10], [10, 10, 20, 20]], [[10, 10, 20, 20], [25, 25, 30, 30]], [0, 1]) == ([-1, 0], [0, 1])
    # no gt
    assert both([[0, 0, 10, 10], [10, 10, 20, 20]], np.zeros((0, 4)), []) == ([-1, -1], [0, 0])
    # the ignore band: IoU 0.45, 0.3, 1
    anchors, gt = [[0, 0, 20, 9], [0, 0, 20, 6], [0, 0, 20, 20]], [[0, 0, 20, 20]]
    assert both(anchors, gt, [2], pos=0.5, neg=0.4)[0] == [-2, -1, 0]
    assert both(anchors, gt, [2], pos=0.5, neg=0.5)[0] == [-1, -1, 0]


def test_helper_refuses_inputs_outside_its_domain():
    ok = [[0, 0, 4, 4]]
    for bad in ([[0, 0, 4.5, 4]], [[0, 0, 33, 4]], [[-1, 0, 4, 4]], [[4, 0, 2, 4]]):
        with pytest.raises(AssertionError):
            match_exact.training_targets(bad, ok, [0])
        with pytest.raises(AssertionError):
            match_exact.training_targets(ok, bad, [0])


def test_fuzz_seeds_agree_and_contain_ties_and_collisions():
    big = 0
    for seed in range(cases.FUZZ_SEEDS):
        case = cases.fuzz_case(seed)
        N, G = len(case["anchors"]), case["boxes"].shape[1]
        assert 1 <= N <= 6000 and 0 <= G <= 600 and (not case["levels"] or sum(case["levels"]) == N)
        stats = []
        _both(case, stats)
        print("seed %d: N %d G %d levels %s, image 0: %s" % (seed, N, G, case["levels"], stats[0]))
        if N >= 500 and G >= 20:
            big += 1
            assert stats[0]["anchor_ties"] > 0 and stats[0]["gt_ties"] > 0 and stats[0]["collisions"] > 0, (seed, stats[0])
    assert big >= 15 and cases.FUZZ_SEEDS >= 20
    assert {len(cases.fuzz_case(s)["levels"]) for s in range(cases.FUZZ_SEEDS)} == {0, 1, 5, 8}
    assert any(0 in cases.fuzz_case(s)["levels"] for s in range(cases.FUZZ_SEEDS))


@pytest.mark.parametrize("values", [cases.MODERATE, cases.PLANTED], ids=["moderate", "extreme"])
@pytest.mark.parametrize("gamma", [2.0, 0.5])
def test_restatement_scalars_stay_within_1e_5_of_float64_on_the_planted_values(ssd, values, gamma):
    """The bound the GPU test applies to ssd_loss's batch scalars is a statement about fp32 arithmetic: the restatement
    alone must meet it on the planted logits and codes."""
    anchors = ssd.AnchorGenerator()(128, 128)
    logits, codes, boxes, labels, num = cases.value_inputs(anchors, 80, [5, 40], seed=21)
    tg = [loss_ref.training_targets(anchors, boxes[b, :num[b]], labels[b, :num[b]]) for b in range(2)]
    reg, cls, m = (np.stack([t[k] for t in tg]) for k in range(3))
    assert cases.plant_logits(logits, cls, m, values) == 2 * 3 * len(values)
    assert cases.plant_codes(codes, reg, m).sum() >= 2 * cases.EQUAL_GT
    with np.errstate(over="ignore"):
        r_losses = loss_ref.batch_losses(logits, codes, anchors, boxes, labels, num, gamma=gamma)[0]
        f64 = loss_ref.losses_f64(logits, codes, anchors, boxes, labels, num, gamma=gamma)
    print(values[-1], gamma, r_losses, f64, np.abs(r_losses - f64) / f64)
    np.testing.assert_allclose(r_losses, f64, rtol=1e-5)
