"""-m gpu: the class-logit screen's signed weight plane and its three-stage ring, and the fill's chunking
(csrc/logit_screen.hip, pack_screen of csrc/weights.hip), at the places where they can go wrong and the cases of
test_gpu_logit_screen.py / test_gpu_logit_screen_sweep.py do not look:

  * weights whose signs alternate in STORED channel order, so that both halves of every 32-bit word of a B fragment go to
    different waves of a pair, and signs in runs of 8 and of 64 channels (whole 16-byte chunks / whole K-steps of one sign);
  * -0, |w| < 2^-14 of both signs, NaN, -inf and +inf in the FIRST K-step (channels 0..63, tap 0) and in the LAST one
    (channels 192..255, tap 8): the ring's prologue and its drain;
  * a row tile with a single valid row (p7 at batch 1) and row tiles that straddle images;
  * column octets with exactly 63, 64, 65 and 129 marked rows (the fill's chunk is 64 rows), and a launch with more chunks
    than blocks, so that a block restages the weights of another column octet.

Every case goes through run_case / check_case of test_gpu_logit_screen.py (or their NaN-tolerant restatement): identical
detections, dense marks inside the screen's, filled logits equal to the dense run's bit for bit -- and inside the envelope of
helpers/logit_screen_ref.py where the case says so.  No case is vacuous: the dense run marks some octets and not all.
Everything the cases are built from comes from the CPU oracle's class towers, nothing from a run of the library."""
import numpy as np
import pytest

from helpers import logit_screen_ref as ref
from test_gpu_logit_screen import BASE, check_case, dense_marks, frames, octets, run_case, scan_lo, screen_marks
from test_gpu_logit_screen_sweep import LEVELS, level_hw, oracle_keep, same_bits, some_not_all

pytestmark = pytest.mark.gpu

KERNEL, BIAS = "class_net/logits/kernel", "class_net/logits/bias"


def phys_of_logical(l):
    """ssd_phys_of_logical of csrc/ssd_internal.h: where logical channel l is stored."""
    l = np.asarray(l)
    r = l & 7
    return (l & ~7) + np.where(r & 1, 4 + (r >> 1), r >> 1)


def envelope_marks(oracle_graph, okey, img, W, p, lo):
    B, H, W_ = img.shape[:3]
    keep = oracle_keep(oracle_graph, okey, img, W, p)
    x = ref.patches([keep["class_tower_%d" % l] for l in LEVELS], level_hw(H, W_))
    return ref.tensor_order(ref.upper_mark_bound(x, W[KERNEL], W[BIAS], lo), B, level_hw(H, W_))


# ---------------------------------------------------------------- signs
def signed_weights(ssd, arrangement):
    """-> params, weights, frames.  `alternate`: the sign of a weight is (-1)^(stored position of its input channel) -- the
    two halves of every 32-bit word of the plane differ in sign.  `runs`: columns 0..239 change sign every 8 channels (a
    16-byte chunk of the plane is of one sign), columns 240..479 every 64 (a whole K-step is)."""
    ch = np.arange(256)
    if arrangement == "alternate":
        p = dict(BASE)
        W = ssd.synthetic_weights(p, seed=1, logits_bias=-8.0)      # (sums of both signs spread wide: about one octet in twelve)
        sign = np.where(phys_of_logical(ch) & 1, -1.0, 1.0).astype(np.float32)[None, None, :, None]
        img = frames(2, 128, 128)
    else:
        p = dict(BASE, min_dimension=256)
        W = ssd.synthetic_weights(p, seed=3, logits_bias=-5.0)
        s8 = np.where((ch >> 3) & 1, -1.0, 1.0)
        s64 = np.where((ch >> 6) & 1, 1.0, -1.0)
        sign = np.concatenate([np.repeat(s8[:, None], 240, 1), np.repeat(s64[:, None], 240, 1)], axis=1).astype(np.float32)[None, None]
        img = frames(3, 256, 384, seed=5)
    W = dict(W)
    W[KERNEL] = (np.abs(W[KERNEL]) * sign).astype(np.float32)
    return p, W, img


@pytest.mark.parametrize("arrangement", ["alternate", "runs"])
def test_signs_within_words_and_in_runs(cuda, ssd, oracle_graph, arrangement):
    p, W, img = signed_weights(ssd, arrangement)
    k = W[KERNEL]
    if arrangement == "alternate":      # stored neighbours 2q, 2q + 1 of every column differ in sign
        stored = k[:, :, np.argsort(phys_of_logical(np.arange(256))), :]
        assert (np.sign(stored[:, :, 0::2]) * np.sign(stored[:, :, 1::2]) <= 0).all() and (stored != 0).mean() > 0.99
    r = run_case(ssd, cuda, ("pipeline signs", arrangement), p, W, img)
    dm, sm = check_case(r, "signs %s" % arrangement)
    some_not_all(dm, arrangement)
    em = envelope_marks(oracle_graph, ("pipeline signs", arrangement), img, W, p, r["lo"])
    print("signs %s: octets %d, dense %d, screened %d, envelope %d" % (arrangement, dm.size, int(dm.sum()), int(sm.sum()), int(em.sum())))
    assert not (sm & ~em).any(), (arrangement, "screened marks outside the envelope", int((sm & ~em).sum()), "of", int(sm.sum()))
    assert 2 * int(em.sum()) < em.size, (arrangement, "the envelope marks", int(em.sum()), "of", em.size)


# ---------------------------------------------------------------- special weights in the first and the last K-step
SPECIAL_COLS = {"negzero": 5, "tiny": 13, "nan": 21, "neginf": 29, "posinf": 37}


def special_weights(ssd, where):
    """K-step (channel block 0, tap 0) or (channel block 3, tap 8).  Column 45's bias sits just above the bound: p7's
    activations are O(1e-3), so the single row of p7 at batch 1 is marked there."""
    W = dict(ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0))
    k, b = W[KERNEL].copy(), W[BIAS].copy()
    (ky, kx), c0 = ((0, 0), 0) if where == "first" else ((2, 2), 192)
    k[ky, kx, c0:c0 + 64:2, SPECIAL_COLS["negzero"]] = -0.0
    k[ky, kx, c0:c0 + 64, SPECIAL_COLS["tiny"]] = np.tile(np.float32([1e-6, -1e-6, 3e-5, -3e-5, 6.0e-5, -6.0e-5, 1e-40, -1e-40]), 8)
    k[ky, kx, c0 + 7, SPECIAL_COLS["nan"]] = np.nan
    k[ky, kx, c0 + 9, SPECIAL_COLS["neginf"]] = -np.inf
    k[ky, kx, c0 + 11, SPECIAL_COLS["posinf"]] = np.inf
    b[SPECIAL_COLS["neginf"]] = 2.0 ** 30       # (test_non_finite_weights_and_bias: a clamped Wn keeps U far above the bound)
    b[45] = scan_lo(BASE["score_threshold"]) + np.float32(0.01)
    W[KERNEL], W[BIAS] = k, b
    return W


def same_but_nan_payload(a, c):
    na, nc = np.isnan(a), np.isnan(c)
    return np.array_equal(na, nc) and np.array_equal(a.view(np.uint32)[~na], c.view(np.uint32)[~nc])


@pytest.mark.parametrize("where", ["first", "last"])
def test_special_weights_in_the_first_and_last_k_step(cuda, ssd, oracle_graph, where):
    """Batch 1 at 128 x 128: p7 is one row, every level but p3 is smaller than a row tile.  NaN payloads are not compared."""
    W = special_weights(ssd, where)
    img = frames(1, 128, 128)
    r = run_case(ssd, cuda, ("pipeline special", where), BASE, W, img)
    for n, a, c in zip(("boxes", "labels", "scores", "num_boxes"), r["scr_out"], r["dense_out"]):
        assert same_bits(a, c), n
    for a, c in zip(r["after_read_out"], r["dense_out"]):
        assert same_bits(a, c), "forward behind the read"
    dm, sm = dense_marks(r), screen_marks(r)
    em = envelope_marks(oracle_graph, ("pipeline special", where), img, W, BASE, r["lo"])
    print("special %s: octets %d, dense %d, screened %d, envelope %d" % (where, dm.size, int(dm.sum()), int(sm.sum()), int(em.sum())))
    some_not_all(dm, where)
    assert not sm.all()
    assert not (dm & ~sm).any(), int((dm & ~sm).sum())
    assert not (sm & ~em).any(), int((sm & ~em).sum())
    d = r["dense_logits"].reshape(-1, 480)
    assert np.isnan(d[:, SPECIAL_COLS["nan"]]).any() and np.isinf(d[:, SPECIAL_COLS["posinf"]]).any()
    assert np.isfinite(d[:, [SPECIAL_COLS["negzero"], SPECIAL_COLS["tiny"]]]).all()
    smo, dmo = sm.reshape(-1, 60), dm.reshape(-1, 60)
    for name in ("nan", "neginf", "posinf"):        # U is NaN or huge wherever the special weight meets a row: marked
        assert smo[:, SPECIAL_COLS[name] // 8].any(), name
    assert dmo[-1, 45 // 8] and smo[-1, 45 // 8], "the single row of p7"
    f, dd = octets(r["filled"]), octets(r["dense_logits"])
    assert same_but_nan_payload(f[sm], dd[sm]), "filled logits differ from the dense run's"
    assert same_but_nan_payload(r["whole"].reshape(-1), r["dense_logits"].reshape(-1)), "class_predictions on demand"
    assert r["rebuilds"] == 0 and r["status"] == r["dense_status"]


# ---------------------------------------------------------------- rows
def test_row_tiles_across_images(cuda, ssd):
    """B = 3 at 128 x 384 with the sign-alternating weights: p4 is 8 x 24, M = 576 -- its first two row tiles end inside an
    image, its third holds 64 valid rows."""
    W = dict(ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0))
    sign = np.where(phys_of_logical(np.arange(256)) & 1, -1.0, 1.0).astype(np.float32)[None, None, :, None]
    W[KERNEL] = (np.abs(W[KERNEL]) * sign).astype(np.float32)
    # (the sums of p4 and above are small beside the bias: column 323 gets its bias ON the bound, so that about half of
    #  the rows of every level are marked there)
    W[BIAS] = W[BIAS].copy()
    W[BIAS][323] = scan_lo(BASE["score_threshold"])
    r = run_case(ssd, cuda, "pipeline rows", BASE, W, frames(3, 128, 384))
    dm, sm = check_case(r, "B=3 128x384, alternating signs")
    some_not_all(dm, "rows")
    off = 16 * 48 * 60
    p4 = dm.reshape(3, -1)[:, off:off + 192 * 60].reshape(3 * 192, 60).any(axis=1)
    for tile in (0, 1, 2):
        rows = np.arange(tile * 256, min(tile * 256 + 256, 576))
        for image in {int(v) for v in rows // 192}:
            assert p4[rows[rows // 192 == image]].any(), ("p4 row tile", tile, "image", image)


# ---------------------------------------------------------------- the fill's chunks
FILL_COUNTS = {2: 63, 9: 64, 17: 65, 30: 129}       # column octet -> marked rows


def fill_weights(ssd, oracle_graph, img):
    """Per chosen column octet one live column: a single weight w > 0 at the centre tap of one input channel, logit =
    w x + bias with bias = scan_lo - 1; the other seven columns are the bias alone.  x is the class tower's output at that
    channel (CPU oracle); w puts the bound between the n-th and the (n+1)-th largest x, in a gap of at least 4 % -- the
    screen's U exceeds the logit by less than 1 % of w x here (2^-9 and the operands' roundings), so exactly the n rows
    with the largest x are marked, by the dense run and by the screen alike."""
    W = dict(ssd.synthetic_weights(BASE, seed=1, logits_bias=-6.0))
    keep = oracle_keep(oracle_graph, "pipeline fill towers", img, W, BASE)
    x = np.concatenate([np.asarray(keep["class_tower_%d" % l], np.float32).reshape(-1, 256) for l in LEVELS], axis=0)
    lo = float(scan_lo(BASE["score_threshold"]))
    k, b = W[KERNEL].copy(), W[BIAS].copy()
    used = set()
    for o, n in FILL_COUNTS.items():
        k[..., 8 * o:8 * o + 8] = 0.0
        b[8 * o:8 * o + 8] = lo - 1.0
        for c in range(256):
            v = np.sort(x[:, c])[::-1]
            if c in used or v.size <= n or not v[n - 1] > 1e-3 or not v[n] < 0.96 * v[n - 1]:
                continue
            used.add(c)
            k[1, 1, c, 8 * o + 3] = np.float32(1.0 / np.sqrt(float(v[n - 1]) * max(float(v[n]), 0.96 * 0.96 * float(v[n - 1]))))
            break
        else:
            raise AssertionError("no channel with a gap behind its %d-th largest value" % n)
    W[KERNEL], W[BIAS] = k, b
    return W


def test_fill_chunks_of_63_64_65_and_129_rows(cuda, ssd, oracle_graph):
    img = frames(2, 128, 128)
    W = fill_weights(ssd, oracle_graph, img)
    r = run_case(ssd, cuda, "pipeline fill", BASE, W, img)
    dm, sm = check_case(r, "fill chunks")
    some_not_all(dm, "fill")
    rows_of = lambda m, o: int(m.reshape(-1, 60)[:, o].sum())
    for o, n in FILL_COUNTS.items():
        print("column octet %d: dense %d, screened %d marked rows (wanted %d)" % (o, rows_of(dm, o), rows_of(sm, o), n))
    for o, n in FILL_COUNTS.items():
        assert rows_of(dm, o) == n and rows_of(sm, o) == n, (o, n, rows_of(dm, o), rows_of(sm, o))


def test_more_chunks_than_blocks_restages_the_weights(cuda, ssd):
    """Threshold 0 at B = 2, 128 x 128 (the run of test_threshold_zero_marks_everything): all 682 rows of all 60 column
    octets are marked, 11 chunks each = 660 chunks for a grid of at most two blocks per CU -- 512 on the 256 CUs of an
    MI355X: blocks 0..147 take a second chunk, 512 further on and so of another column octet."""
    p = dict(BASE, score_threshold=0.0)
    W = ssd.synthetic_weights(p, seed=1, logits_bias=-7.5)
    r = run_case(ssd, cuda, "thr0", p, W, frames(2, 128, 128))
    dm, sm = check_case(r, "threshold 0")
    assert sm.all()
    chunks = 60 * -(-682 // 64)
    cus = cuda.cuda.get_device_properties(0).multi_processor_count
    assert chunks > 2 * cus, (chunks, cus)
