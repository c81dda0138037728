"""-m gpu: the class logits as screen + fill (csrc/logit_screen.hip, option logits_screen) against the dense launch of the
same engine: identical detections, a sound screen (every octet the dense run marks is marked), exact logits at every
marked octet, and the whole tensor on demand.

Shapes: B = 2 at 128 x 128 (p3 16x16 .. p7 1x1: levels smaller than a tile, rows past M) and B = 3 at 256 x 384 (p3 spans
several row tiles, per-level offsets differ).  One engine per case serves both forms (the option drops the plans, not
the weights); a case's runs are made once and shared by the tests that read them.

Option logits_screen = 2 is the screened plan with the logits tensor filled with 0xff bytes first, so that
get_tensor("class_logits_filled") -- the tensor as the fill left it -- shows which octets were marked."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = {"backbone": "mobilenet", "depth_multiplier": 1.0, "num_classes": 80, "score_threshold": 0.15,
        "iou_threshold": 0.6, "max_boxes_per_class": 25, "min_dimension": 128}
LEVELS = (3, 4, 5, 6, 7)


def scan_lo(thr):
    """conservative_logit_bound of csrc/plan.hip."""
    if not thr > 0.0:
        return np.float32(-np.inf)
    l = math.log(thr / (1.0 - thr))
    return np.float32(l - 1e-3 * (1.0 + abs(l)))


def frames(B, H, W, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def scaled_tower(W, gain):
    """The class tower's last batch norm scaled: its output (the logits convolution's input) times `gain`."""
    out = dict(W)
    for l in LEVELS:
        for leaf in ("gamma", "beta"):
            n = "class_net/batch_norm_3_for_level_%d/%s" % (l, leaf)
            out[n] = (W[n] * np.float32(gain)).astype(np.float32)
    return out


def signed_columns(W):
    out = dict(W)
    k = W["class_net/logits/kernel"].copy()
    k[..., 5] = -np.abs(k[..., 5])
    k[..., 6] = np.abs(k[..., 6])
    k[..., 477] = -np.abs(k[..., 477])
    out["class_net/logits/kernel"] = k
    b = W["class_net/logits/bias"].copy()
    b[6] = -9.0          # (the all-positive column sits ~ +4 above the others: keep it near the bound)
    out["class_net/logits/bias"] = b
    return out


_RUNS = {}


def run_case(ssd, cuda, key, params, W, img, repeats=0, forward=None):
    """Dense run, then screened run of one engine.  Returns everything the tests compare.  `forward(eng)`: the forward
    through another entry point than eng.forward(img) -> the four output tensors."""
    if key in _RUNS:
        return _RUNS[key]
    eng = ssd.Engine(params, W)
    if forward is None:
        x = cuda.from_numpy(img).cuda()

        def forward(eng):
            return eng.forward(x)
    r = {"lo": scan_lo(params["score_threshold"])}
    eng.set_option("logits_screen", 0)
    r["dense_out"] = [t.cpu().numpy() for t in forward(eng)]
    r["dense_logits"] = eng.get_tensor("class_predictions")
    r["dense_status"] = eng.status()
    eng.set_option("logits_screen", 2)
    r["scr_out"] = [t.cpu().numpy() for t in forward(eng)]
    r["filled"] = eng.get_tensor("class_logits_filled").copy()
    r["repeat_same"] = True
    for _ in range(repeats):
        again = [t.cpu().numpy() for t in forward(eng)]
        r["repeat_same"] = r["repeat_same"] and all(np.array_equal(a, b) for a, b in zip(again, r["scr_out"]))
    st0 = eng.plan_cache_stats()
    r["whole"] = eng.get_tensor("class_predictions")
    r["after_read_out"] = [t.cpu().numpy() for t in forward(eng)]
    st1 = eng.plan_cache_stats()
    r["rebuilds"] = st1["misses"] - st0["misses"]
    r["status"] = eng.status()
    eng.close()
    _RUNS[key] = r
    return r


def octets(a):
    return a.reshape(-1, 8)


def dense_marks(r):
    """The octets the dense launch's epilogue marks: max of the octet >= scan_lo, a NaN dropped (fmaxf)."""
    with np.errstate(invalid="ignore"):
        return (np.fmax.reduce(octets(r["dense_logits"]), axis=1) >= r["lo"])


def screen_marks(r):
    return (octets(r["filled"]).view(np.uint32) != 0xFFFFFFFF).any(axis=1)


def check_case(r, what):
    names = ("boxes", "labels", "scores", "num_boxes")
    for n, a, b in zip(names, r["scr_out"], r["dense_out"]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), (what, n)
    dm, sm = dense_marks(r), screen_marks(r)
    print("%s: octets %d, dense marks %d, screened marks %d (ratio %.3f), detections %s"
          % (what, dm.size, int(dm.sum()), int(sm.sum()), sm.sum() / max(1, dm.sum()), r["dense_out"][3].tolist()))
    assert not (dm & ~sm).any(), (what, "octets the dense run marks and the screen missed", int((dm & ~sm).sum()))
    f, d = octets(r["filled"]).view(np.uint32), octets(r["dense_logits"]).view(np.uint32)
    assert np.array_equal(f[sm], d[sm]), (what, "filled logits differ from the dense run's")
    assert np.array_equal(r["whole"].view(np.uint32), r["dense_logits"].view(np.uint32)), (what, "class_predictions on demand")
    for a, b in zip(r["after_read_out"], r["dense_out"]):
        assert np.array_equal(a, b), (what, "forward behind the read")
    assert r["rebuilds"] == 0, what
    assert r["dense_status"] == 0 and r["status"] == 0, what
    return dm, sm


def border_and_tail_marked(sm, B, hw):
    """Marked octets on the zero-padded border of every level, and in the last partial 256-row tile of every level."""
    per_img = sum(h * w for h, w in hw) * 60
    m = sm.reshape(B, per_img)
    off = 0
    for h, w in hw:
        lvl = m[:, off:off + h * w * 60].reshape(B, h, w, 60)
        border = np.zeros((h, w), bool)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
        assert lvl[:, border].any(), ("no marked octet on the border of level", h, w)
        rows = lvl.reshape(B * h * w, 60)
        tail = rows[(B * h * w - 1) // 256 * 256:]
        assert tail.any(), ("no marked octet in the last row tile of level", h, w)
        off += h * w * 60


HW128 = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]


@pytest.mark.parametrize("bias", [-7.5, -math.log(99.0)])
def test_same_results_sound_screen_exact_fill(cuda, ssd, bias):
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=bias)
    r = run_case(ssd, cuda, ("b2", bias), BASE, W, frames(2, 128, 128), repeats=20 if bias == -7.5 else 0)
    dm, sm = check_case(r, "B=2 128x128 bias %.3f" % bias)
    assert r["repeat_same"], "a repeated screened forward differs from the first"


def test_threshold_zero_marks_everything(cuda, ssd):
    p = dict(BASE, score_threshold=0.0)
    W = ssd.synthetic_weights(p, seed=1, logits_bias=-7.5)
    r = run_case(ssd, cuda, "thr0", p, W, frames(2, 128, 128))
    dm, sm = check_case(r, "threshold 0")
    assert sm.all() and dm.all()
    border_and_tail_marked(sm, 2, HW128)


def test_three_images_256x384(cuda, ssd):
    p = dict(BASE, min_dimension=256)
    W = ssd.synthetic_weights(p, seed=3, logits_bias=-1.5)       # (many marked octets: borders and tails of every level among them)
    r = run_case(ssd, cuda, "b3", p, W, frames(3, 256, 384, seed=5))
    dm, sm = check_case(r, "B=3 256x384")
    border_and_tail_marked(sm, 3, [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)])


@pytest.mark.parametrize("case", ["overflow", "subnormal", "zero", "signed_columns"])
def test_adversarial_inputs(cuda, ssd, case):
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-4.0)
    if case == "overflow":
        W = scaled_tower(W, 3.0e5)          # activations O(1) -> O(3e5): past 65504, inf in the f16 plane
    elif case == "subnormal":
        W = scaled_tower(W, 1.0e-6)         # below 2^-14 throughout
        W["class_net/logits/bias"] = np.full_like(W["class_net/logits/bias"], scan_lo(0.15))
    elif case == "zero":
        W = scaled_tower(W, 0.0)
        W["class_net/logits/bias"] = np.full_like(W["class_net/logits/bias"], scan_lo(0.15))
    else:
        W = signed_columns(W)
    r = run_case(ssd, cuda, case, BASE, W, frames(2, 128, 128))
    dm, sm = check_case(r, case)
    if case == "overflow":
        tower_max = float(np.abs(r["dense_logits"]).max())
        assert tower_max > 1e3, tower_max
    if case == "zero":
        assert dm.all()                     # every logit IS the bound (the bias)


def test_logits_within_one_ulp_of_the_bound(cuda, ssd, oracle_graph):
    """Per chosen column the bias is solved on the CPU oracle so that one logit lands exactly on scan_lo, one ulp below
    it, or one ulp above it: the screen must mark the first and the third (the dense run does), whatever it does with the second."""
    W = ssd.synthetic_weights(BASE, seed=1, logits_bias=-7.5)
    img = frames(2, 128, 128)
    W0 = dict(W)
    W0["class_net/logits/bias"] = np.zeros_like(W["class_net/logits/bias"])
    keep = {}
    oracle_graph.forward(img, W0, BASE, keep=keep)
    acc = np.asarray(keep["class_predictions"], np.float32).reshape(2, -1, 480)       # bias 0: the chain's value itself
    lo = scan_lo(BASE["score_threshold"])
    targets = {0: lo, 1: np.nextafter(lo, np.float32(-np.inf)), 2: np.nextafter(lo, np.float32(np.inf))}
    rng = np.random.default_rng(11)
    bias = W["class_net/logits/bias"].copy()
    placed = []
    for col in range(0, 480, 7):
        b, pos = int(rng.integers(0, 2)), int(rng.integers(0, acc.shape[1]))
        a, t = acc[b, pos, col], targets[col % 3]
        guess = np.float32(t - a)
        for step in range(-8, 9):             # fl32(a + bias) == t: the neighbours of t - a
            cand = guess
            for _ in range(abs(step)):
                cand = np.nextafter(cand, np.float32(np.inf if step > 0 else -np.inf))
            if np.float32(a + cand) == t:
                bias[col] = cand
                placed.append((b, pos, col, t))
                break
    assert len(placed) >= 40, len(placed)
    W1 = dict(W)
    W1["class_net/logits/bias"] = bias
    r = run_case(ssd, cuda, "near_lo", BASE, W1, img)
    dm, sm = check_case(r, "logits within 1 ulp of the bound")
    d = r["dense_logits"].reshape(2, -1, 480)
    hit = sum(1 for b, pos, col, t in placed if d[b, pos, col] == t)
    print("placed %d logits, %d landed on their target in the dense run" % (len(placed), hit))
    assert hit >= len(placed) // 2, (hit, len(placed))
