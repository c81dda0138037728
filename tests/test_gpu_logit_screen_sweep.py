"""-m gpu: the class-logit screen (csrc/logit_screen.hip, pack_screen of csrc/weights.hip) past the one network and the one
read path of test_gpu_logit_screen.py: other head widths (one partial column tile .. 126 column octets), widths that must
stay dense, batch 1 and row tiles that straddle images, sub-batch plans, the device-side read of the logits, mixed-size
batches, the automatic rule on either side of SSD_SCREEN_MIN_ROWS, non-finite weights, a threshold that marks nothing --
and the screen's TIGHTNESS: its marks lie inside an envelope computed from the CPU oracle's class towers alone
(helpers/logit_screen_ref.py), so a screen that marks far too much fails here and not only in the benchmark.

Every case goes through run_case / check_case of test_gpu_logit_screen.py (identical detections, sound screen, exact fill,
the whole tensor on demand, the forward behind the read, no plan rebuild, status 0) and asserts that it is not vacuous:
the dense run marks some octets and not all.  Every comparison is bit-exact or a set containment."""
import numpy as np
import pytest

from helpers import logit_screen_ref as ref
from test_gpu_logit_screen import (BASE, check_case, dense_marks, frames, octets, run_case, scaled_tower,
                                   scan_lo, screen_marks)
from test_gpu_mixed_batch import TINY_SIZES, _frame

pytestmark = pytest.mark.gpu

LEVELS = (3, 4, 5, 6, 7)


def level_hw(H, W):
    return [(H >> l, W >> l) for l in LEVELS]


def some_not_all(dm, what):
    assert 0 < int(dm.sum()) < dm.size, (what, "dense marks", int(dm.sum()), "of", dm.size)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                 b.view(np.uint32) if b.dtype == np.float32 else b)


def postprocess_launches(eng, forward):
    """Launches of profile class `postprocess` (the screen's launches are booked there) in one forward of a warm plan."""
    forward()
    eng.profile_reset()
    eng.profile_enable(True)
    forward()
    eng.profile_enable(False)
    return eng.profile_read()["postprocess"]["launches"]


_ORACLE = {}


def oracle_keep(oracle_graph, key, img, W, params):
    """The oracle's intermediates of one (weights, frames) pair: computed once, read by every test that needs them."""
    if key not in _ORACLE:
        keep = {}
        oracle_graph.forward(img, W, params, keep=keep)
        _ORACLE[key] = {n: keep[n] for n in ["class_predictions"] + ["class_tower_%d" % l for l in LEVELS]}
    return _ORACLE[key]


# ---------------------------------------------------------------- column tiling: head widths other than 480
@pytest.mark.parametrize("C", [4, 20, 84, 88, 168])
def test_class_counts(cuda, ssd, oracle_graph, C):
    """6 C logit columns: 24 and 120 (one partial column tile), 504 (4 tiles, the last 120 wide), 528 (a fifth tile of 16
    columns), 1008 (8 tiles, 126 column octets).  The last column's bias sits on scan_lo, so that the last octet of the last
    column tile is marked in about half of the rows; the dense run that check_case compares with is itself the oracle's."""
    p = dict(BASE, num_classes=C, max_boxes_per_class=5)
    W = ssd.synthetic_weights(p, seed=1, logits_bias=-6.0)
    W["class_net/logits/bias"][-1] = scan_lo(p["score_threshold"])
    img = frames(2, 128, 128)
    r = run_case(ssd, cuda, ("classes", C), p, W, img)
    dm, sm = check_case(r, "C = %d" % C)
    some_not_all(dm, C)
    want = oracle_keep(oracle_graph, ("classes", C), img, W, p)["class_predictions"]
    assert same_bits(r["dense_logits"].reshape(-1), np.asarray(want, np.float32).reshape(-1)), (C, "dense logits vs the oracle")
    NO = 6 * C // 8
    first_of_last_tile = (6 * C - 1) // 128 * 16
    dmo, smo = dm.reshape(-1, NO), sm.reshape(-1, NO)
    assert dmo[:, NO - 1].any() and smo[:, NO - 1].any(), (C, "last column octet")
    assert dmo[:, first_of_last_tile:].any() and smo[:, first_of_last_tile:].any(), (C, "last column tile")
    assert not dmo[:, NO - 1].all(), (C, "the last octet is marked in every row")


@pytest.mark.parametrize("C", [3, 90])
def test_ineligible_width_stays_dense(cuda, ssd, C):
    """6 C is no multiple of 8 (18, 540 columns): no octet bitmap, so logits_screen = 1 must leave the dense plan in place --
    same launches, same bits."""
    p = dict(BASE, num_classes=C, max_boxes_per_class=5)
    W = ssd.synthetic_weights(p, seed=1, logits_bias=-4.0)
    x = cuda.from_numpy(frames(2, 128, 128)).cuda()
    eng = ssd.Engine(p, W)
    got = {}
    for opt in (0, 1):
        eng.set_option("logits_screen", opt)
        launches = postprocess_launches(eng, lambda: eng.forward(x))
        out = [t.cpu().numpy() for t in eng.forward(x)]
        got[opt] = (out, eng.get_tensor("class_predictions"), launches, eng.status())
    eng.close()
    assert int(got[0][0][3].sum()) > 0, "no detections: the comparison would be vacuous"
    for a, b in zip(got[1][0], got[0][0]):
        assert same_bits(a, b), C
    assert same_bits(got[1][1], got[0][1]), C
    assert got[1][2] == got[0][2] and got[0][2] > 0, (C, got[0][2], got[1][2])
    assert got[0][3] == 0 and got[1][3] == 0


# ---------------------------------------------------------------- rows: batch 1, tiles that straddle images
@pytest.mark.parametrize("B,H,W_", [(1, 128, 128), (3, 128, 384)])
def test_batch_one_and_row_tiles_across_images(cuda, ssd, B, H, W_):
    """B = 1 at 128 x 128: every level but p3 is smaller than a 256-row tile.  B = 3 at 128 x 384: p4 is 8 x 24, M = 576 -- the
    first and the second row tile of p4 end inside an image."""
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0)
    r = run_case(ssd, cuda, ("rows", B, H, W_), BASE, W, frames(B, H, W_))
    dm, sm = check_case(r, "B=%d %dx%d" % (B, H, W_))
    some_not_all(dm, (B, H, W_))
    per_img = dm.reshape(B, -1)
    assert per_img.any(axis=1).all(), "an image without a marked octet"
    if B == 3:          # the straddling tiles of p4 hold marks on both sides of an image boundary
        off = 16 * 48 * 60
        p4 = dm.reshape(B, -1)[:, off:off + 192 * 60].reshape(B * 192, 60).any(axis=1)
        for tile in (0, 1):
            rows = np.arange(tile * 256, tile * 256 + 256)
            assert len({int(v) for v in rows // 192}) == 2
            for image in {int(v) for v in rows // 192}:
                assert p4[rows[rows // 192 == image]].any(), ("p4 row tile", tile, "image", image)


# ---------------------------------------------------------------- sub-batch plans
@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_sub_batch_plans_screened(cuda, ssd, libopt, backbone):
    """Option nsub = 3 splits B = 5 into plans of 2 + 2 + 1 images, each with its own ScreenArgs, counters and row lists
    (ShuffleNet: the head towers in a block of their own).  Every image gets the marks it gets in the single plan of 5."""
    p = dict(BASE, backbone=backbone)
    W = ssd.synthetic_weights(p, seed=12, logits_bias=-6.0)
    img = np.random.default_rng(6).integers(0, 256, (5, 128, 128, 3), dtype=np.uint8)
    one = run_case(ssd, cuda, ("nsub", backbone, 1), p, W, img)
    libopt(nsub=3)
    sub = run_case(ssd, cuda, ("nsub", backbone, 3), p, W, img)
    dm1, sm1 = check_case(one, "one plan of 5, " + backbone)
    dm3, sm3 = check_case(sub, "plans of 2 + 2 + 1, " + backbone)
    some_not_all(dm3, backbone)
    assert dm3.reshape(5, -1).any(axis=1).all(), "an image without a marked octet"
    for a, b in zip(sub["dense_out"], one["dense_out"]):
        assert same_bits(a, b), backbone
    assert same_bits(sub["dense_logits"], one["dense_logits"]), backbone
    for b in range(5):
        assert np.array_equal(sm3.reshape(5, -1)[b], sm1.reshape(5, -1)[b]), (backbone, "marks of image", b)


# ---------------------------------------------------------------- the device-side read
@pytest.mark.parametrize("second_stream", [False, True])
def test_get_tensor_dev_behind_a_screened_forward(cuda, ssd, second_stream):
    """ssd_get_tensor_dev("class_predictions") runs the dense launch on the CALLER's stream, without a device
    synchronisation.  Option 2 fills the tensor with 0xff bytes before every screened forward, so nothing an earlier
    forward left can pass for the result."""
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0)
    x = cuda.from_numpy(frames(2, 128, 128)).cuda()
    eng = ssd.Engine(BASE, W)
    eng.set_option("logits_screen", 0)
    dense_out = [t.cpu().numpy() for t in eng.forward(x)]
    dense = eng.get_tensor("class_predictions")
    eng.set_option("logits_screen", 2)
    side = cuda.cuda.Stream() if second_stream else None          # (a torch stream is non-blocking)

    def read():
        if side is None:
            t = eng.get_tensor_dev("class_predictions", dense.shape)
            cuda.cuda.current_stream().synchronize()
            return t.cpu().numpy()
        side.wait_stream(cuda.cuda.current_stream())               # behind the forward
        with cuda.cuda.stream(side):
            t = eng.get_tensor_dev("class_predictions", dense.shape)
        side.synchronize()                                         # the next forward overwrites what the dense launch reads
        return t.cpu().numpy()
    out1 = [t.cpu().numpy() for t in eng.forward(x)]
    filled = eng.get_tensor("class_logits_filled")
    sm = (octets(filled).view(np.uint32) != 0xFFFFFFFF).any(axis=1)
    some_not_all(sm, "screened marks")                             # (the read has something to make whole)
    first = read()
    out2 = [t.cpu().numpy() for t in eng.forward(x)]
    second = read()
    again = read()                                                 # (already whole: no second dense launch, the same tensor)
    out3 = [t.cpu().numpy() for t in eng.forward(x)]
    status = eng.status()
    eng.close()
    assert int(dense_out[3].sum()) > 0
    for got in (first, second, again):
        assert same_bits(got, dense), "class_predictions on the device"
    for out in (out1, out2, out3):
        for a, b in zip(out, dense_out):
            assert same_bits(a, b), "detections around the read"
    assert status == 0


# ---------------------------------------------------------------- mixed-size batches
def test_mixed_frames_screened(cuda, ssd):
    """forward_mixed / detect_host_mixed (per-image box scalers; five source sizes that share the network shape 128 x 256)
    on a screened plan: the outputs of option 0 bit for bit, under option 1 and through check_case under option 2."""
    W = ssd.synthetic_weights(BASE, seed=5, logits_bias=-6.0)
    fr = [_frame(h, w) for h, w in TINY_SIZES]
    dev = [cuda.from_numpy(f).cuda() for f in fr]
    r = run_case(ssd, cuda, "mixed", BASE, W, None, forward=lambda eng: eng.forward_mixed(dev))
    dm, sm = check_case(r, "forward_mixed")
    some_not_all(dm, "mixed")
    assert int(r["dense_out"][3].sum()) > 0 and dm.reshape(5, -1).any(axis=1).all()
    eng = ssd.Engine(BASE, W)
    got = {}
    for opt in (0, 1):
        eng.set_option("logits_screen", opt)
        got[opt] = ([t.cpu().numpy() for t in eng.forward_mixed(dev)], [np.array(v) for v in eng.detect_host_mixed(fr)])
    status = eng.status()
    eng.close()
    for k in range(4):
        assert same_bits(got[1][0][k], got[0][0][k]) and same_bits(got[1][1][k], got[0][1][k]), k
        assert same_bits(got[0][0][k], r["dense_out"][k]) and same_bits(got[0][1][k], r["dense_out"][k]), k
    assert status == 0


# ---------------------------------------------------------------- the automatic rule
def test_automatic_rule_switches_at_the_row_threshold(cuda, ssd):
    """A 128 x 128 frame has 256 + 64 + 16 + 4 + 1 = 341 rows: B = 96 gives 32 736 < SSD_SCREEN_MIN_ROWS = 32 768 <= 33 077 of
    B = 97.  With the option unset the plan of 96 is the dense one and the plan of 97 the screened one -- told apart by the
    launches of profile class `postprocess`, which are observed under options 0 and 1 on the same engine.  B = 97 also has a
    level with more images than rows per image (p7: M = 97, P = 1)."""
    assert 96 * 341 < 32768 <= 97 * 341
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0)
    # p7 of the synthetic network is nearly dead (its logits are the bias + O(1e-3)): column 323 is one whose p7 sum changes
    # sign between these frames, so with its bias ON the bound some images mark p7 and some do not
    W["class_net/logits/bias"][323] = scan_lo(BASE["score_threshold"])
    img = frames(97, 128, 128)
    x = {97: cuda.from_numpy(img).cuda()}
    x[96] = x[97][:96].contiguous()
    eng = ssd.Engine(BASE, W)
    n = {}
    for opt in ("auto", 0, 1):
        if opt != "auto":
            eng.set_option("logits_screen", opt)
        for B in (96, 97):
            n[opt, B] = postprocess_launches(eng, lambda: eng.forward(x[B]))
    eng.close()
    print("postprocess launches:", n)
    for B in (96, 97):
        assert n[0, B] != n[1, B], ("the dense and the screened plan show the same launch count", B, n)
    assert n["auto", 96] == n[0, 96], n
    assert n["auto", 97] == n[1, 97], n
    assert n["auto", 96] != n[1, 96] and n["auto", 97] != n[0, 97], n          # the plans of 96 and of 97 differ in kind
    r = run_case(ssd, cuda, "b97", BASE, W, img)
    dm, sm = check_case(r, "B=97 128x128")
    some_not_all(dm, "B=97")
    p7 = dm.reshape(97, -1)[:, -60:]
    assert p7.any() and not p7[:, 323 // 8].all(), ("marked p7 octets of column 323", int(p7[:, 323 // 8].sum()), "of 97")


# ---------------------------------------------------------------- tightness
def tight_case(ssd, name):
    """-> key of the run, params, weights, frames, key of the oracle run (the towers do not depend on the threshold)."""
    if name in ("overflow", "subnormal"):       # the weight sets and the runs of test_adversarial_inputs
        W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-4.0)
        if name == "overflow":
            W = scaled_tower(W, 3.0e5)
        else:
            W = scaled_tower(W, 1.0e-6)
            W["class_net/logits/bias"] = np.full_like(W["class_net/logits/bias"], scan_lo(0.15))
        return name, BASE, W, frames(2, 128, 128), ("tight", name)
    shape, C, thr = name
    if shape == "b2":
        p = dict(BASE, num_classes=C, score_threshold=thr)
        return ("tight",) + name, p, ssd.synthetic_weights(p, seed=1, logits_bias=-6.0), frames(2, 128, 128), ("tight", shape, C)
    p = dict(BASE, min_dimension=256, score_threshold=thr)
    return ("tight",) + name, p, ssd.synthetic_weights(p, seed=3, logits_bias=-5.0), frames(3, 256, 384, seed=5), ("tight", shape, C)


TIGHT = [(s, C, thr) for s, C in (("b2", 80), ("b2", 20), ("b3", 80)) for thr in (0.15, 0.5)] + ["overflow", "subnormal"]


@pytest.mark.parametrize("name", TIGHT, ids=lambda n: n if isinstance(n, str) else "%s-C%d-thr%g" % n)
def test_screen_is_tight(cuda, ssd, oracle_graph, name):
    """dense marks <= screened marks <= envelope.  The envelope (helpers/logit_screen_ref.py, upper_mark_bound) is what a
    correct screen can mark at most: the exact sums of the directed-rounded operands, the matrix pipe's worst case in any
    order, pack_screen's constant one ulp up, four ulps for the fp32 epilogue -- from the oracle's class towers, not from a
    run of the library.  Garbage in the f16 plane's padding, Wn rows of the wrong half-tile or a cst that is too large
    push marks outside it.  In the plain cases the envelope itself marks less than half of the octets (a property of the
    chosen bias), so the cap means something; the overflow set (inf in the f16 plane: NaN sums, which mark) and the
    subnormal set (every logit on the bound) are there for the containment alone."""
    key, p, W, img, okey = tight_case(ssd, name)
    r = run_case(ssd, cuda, key, p, W, img)
    dm, sm = check_case(r, "tightness %s" % (name,))
    B, H, W_ = img.shape[:3]
    keep = oracle_keep(oracle_graph, okey, img, W, p)
    x = ref.patches([keep["class_tower_%d" % l] for l in LEVELS], level_hw(H, W_))
    em = ref.tensor_order(ref.upper_mark_bound(x, W["class_net/logits/kernel"], W["class_net/logits/bias"], r["lo"]), B, level_hw(H, W_))
    assert em.shape == sm.shape
    print("tightness %s: octets %d, dense %d, screened %d, envelope %d" % (name, dm.size, int(dm.sum()), int(sm.sum()), int(em.sum())))
    assert same_bits(r["dense_logits"].reshape(-1), np.asarray(keep["class_predictions"], np.float32).reshape(-1)), "dense logits vs the oracle"
    assert not (dm & ~sm).any(), (name, "dense marks outside the screen's", int((dm & ~sm).sum()))
    assert not (sm & ~em).any(), (name, "screened marks outside the envelope", int((sm & ~em).sum()), "of", int(sm.sum()))
    assert not (dm & ~em).any(), name
    assert int(dm.sum()) > 0, name
    if not isinstance(name, str):
        some_not_all(dm, name)
        assert 2 * int(em.sum()) < em.size, (name, "the envelope marks", int(em.sum()), "of", em.size)


# ---------------------------------------------------------------- non-finite operands
def test_non_finite_weights_and_bias(cuda, ssd):
    """pack_screen's branches: a NaN weight (column 5: into Wp, every U of the column is NaN), a -inf weight (column 13:
    clamped to 65504 in Wn) and a NaN bias (column 21: cst is NaN).  A NaN U marks.  Column 13's exact logit is -inf or NaN
    in every row, and where its input is positive the clamped term rightly pulls U down by 65504 x; its bias is 2^30, which
    no such term reaches at these activations (O(1)), so U stays far above the bound and the octet must be marked in
    every row -- an unclamped Wn (inf) would give U = -inf or NaN there instead.  NaN payloads are not compared."""
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0)
    k = W["class_net/logits/kernel"].copy()
    k[1, 1, 7, 5] = np.nan
    k[0, 2, 100, 13] = -np.inf
    b = W["class_net/logits/bias"].copy()
    b[13] = 2.0 ** 30
    b[21] = np.nan
    W["class_net/logits/kernel"], W["class_net/logits/bias"] = k, b
    r = run_case(ssd, cuda, "nonfinite", BASE, W, frames(2, 128, 128))
    for n, a, c in zip(("boxes", "labels", "scores", "num_boxes"), r["scr_out"], r["dense_out"]):
        assert same_bits(a, c), n
    for a, c in zip(r["after_read_out"], r["dense_out"]):
        assert same_bits(a, c), "forward behind the read"
    assert int(r["dense_out"][3].sum()) > 0
    d = r["dense_logits"].reshape(-1, 480)
    assert np.isnan(d[:, 5]).all() and np.isnan(d[:, 21]).all() and (np.isnan(d[:, 13]) | (d[:, 13] == -np.inf)).all()
    assert np.isfinite(np.delete(d, [5, 13, 21], axis=1)).all()
    assert float(np.abs(np.delete(d, [5, 13, 21], axis=1)).max()) < 100.0          # activations O(1): 65504 x << 2^30
    dm, sm = dense_marks(r), screen_marks(r)
    print("non-finite: octets %d, dense marks %d, screened marks %d" % (dm.size, int(dm.sum()), int(sm.sum())))
    some_not_all(dm, "non-finite")
    assert not sm.all()
    assert not (dm & ~sm).any(), int((dm & ~sm).sum())
    smo = sm.reshape(-1, 60)
    for col in (5, 13, 21):
        assert smo[:, col // 8].all(), ("octet of column", col, "unmarked in rows", int((~smo[:, col // 8]).sum()))

    def same_but_nan_payload(a, c):
        na, nc = np.isnan(a), np.isnan(c)
        return np.array_equal(na, nc) and np.array_equal(a.view(np.uint32)[~na], c.view(np.uint32)[~nc])
    f, dd = octets(r["filled"]), octets(r["dense_logits"])
    assert same_but_nan_payload(f[sm], dd[sm]), "filled logits differ from the dense run's"
    assert same_but_nan_payload(r["whole"].reshape(-1), r["dense_logits"].reshape(-1)), "class_predictions on demand"
    assert r["rebuilds"] == 0
    assert r["status"] == r["dense_status"]


# ---------------------------------------------------------------- nothing marked
def test_threshold_with_no_marks(cuda, ssd):
    """score_threshold 0.999: scan_lo = 6.9, far above the logits (bias -6) -- few or no marks, so the compaction finds (next
    to) no row and the fill launch has (next to) no chunk.  Same detections, and the tensor on demand is still whole."""
    p = dict(BASE, score_threshold=0.999)
    W = ssd.synthetic_weights(p, seed=1, logits_bias=-6.0)
    r = run_case(ssd, cuda, "thr999", p, W, frames(2, 128, 128))
    dm, sm = check_case(r, "threshold 0.999")
    assert int(sm.sum()) * 1000 < sm.size, int(sm.sum())
    assert np.isfinite(r["whole"]).all()
