"""The JPEG decoder where coefficients are loud (include/ssd_hip.h, block "the JPEG decoder", "Pinned streams"), without a GPU: the
rule's three limbs in exact integers (jpeg_ref.ranges / pinned), the files of tests/helpers/jpeg_loud.py on both sides of it -- the
restatement equals PIL bit for bit on every pinned file, ssd_jpeg_entropy returns the restatement's coefficients for it and
SSD_ERR_UNSUPPORTED for every other --, the colour clamp at its corners, the upsampling's rounding biases where they decide, the
soundness of the host stage's block-sum screen, and the writer of crafted files (tests/helpers/jpeg_craft.py) against PIL."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.helpers import jpeg_cases, jpeg_craft, jpeg_loud, jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, -5


@pytest.fixture(scope="module")
def entropy(ssd):
    """entropy(blob) -> (status, coef, quant) of ssd_jpeg_info_read + ssd_jpeg_entropy; the parser accepts every file here."""
    from importlib import import_module
    L, lib = import_module("ssd_amd._lib"), ssd.lib()

    def run(blob):
        info = L.SsdJpegInfo()
        assert lib.ssd_jpeg_info_read(blob, len(blob), ctypes.byref(info)) == OK
        coef, quant = np.full(int(info.coef_count), 0x5A5A, np.int16), np.full(64 * int(info.components), 0xA5A5, np.uint16)
        return lib.ssd_jpeg_entropy(blob, len(blob), ctypes.byref(info), coef.ctypes.data, quant.ctypes.data), coef, quant
    return run


def either_pil_or_refused(entropy, files):
    """Every file: pinned -> the restatement equals PIL and the host stage returns its coefficients and tables; else refused.
    -> (pinned, refused) counts."""
    counts = [0, 0]
    for name, blob, p in files:
        rc, coef, quant = entropy(blob)
        if jpeg_ref.pinned(p):
            assert np.array_equal(jpeg_ref.pixels(p), jpeg_cases.pil_rgb(blob)), "%s: pinned by the rule, and differs from PIL" % name
            assert rc == OK, "%s: pinned, status %d" % (name, rc)
            assert np.array_equal(coef, np.concatenate([c.reshape(-1) for c in p["coef"]])), name
            assert np.array_equal(quant, p["quant"].reshape(-1)), name
            counts[0] += 1
        else:
            assert rc == UNSUPPORTED, "%s: not pinned (ranges %s), status %d" % (name, jpeg_ref.ranges(p), rc)
            counts[1] += 1
    return tuple(counts)


# ----------------------------------------------------------------------------- the writer
def test_writer_round_trips_every_plainly_coded_case():
    n = 0
    for name, blob in jpeg_cases.cases():
        if name.endswith("optimize"):
            continue
        p = jpeg_ref.parse(blob)
        again = jpeg_craft.write(p["coef"], p["quant"], p["height"], p["width"], name.split("-")[1], p["restart"])
        q = jpeg_ref.parse(again)
        assert all(q[k] == p[k] for k in ("height", "width", "components", "h", "v", "mcus_x", "mcus_y", "restart")), name
        assert all(np.array_equal(a, b) for a, b in zip(p["coef"], q["coef"])) and np.array_equal(p["quant"], q["quant"]), name
        assert np.array_equal(jpeg_cases.pil_rgb(again), jpeg_cases.pil_rgb(blob)), name
        n += 1
    assert n == 360


def test_writer_refuses_what_baseline_cannot_code():
    q = np.ones(64, np.uint16)

    def block(k, value):
        b = np.zeros((1, 64), np.int32)
        b[0, k] = value
        return [b]
    for k, value in ((5, 1023), (5, -1023), (0, 2047), (0, -2047)):
        p = jpeg_ref.parse(jpeg_craft.write(block(k, value), q, 8, 8, "gray"))
        assert p["coef"][0][0, k] == value
    for k, value in ((5, 1024), (63, -1024), (0, 2048), (0, -2048)):
        with pytest.raises(ValueError):
            jpeg_craft.write(block(k, value), q, 8, 8, "gray")
    two = np.zeros((2, 64), np.int32)
    two[0, 0], two[1, 0] = 1500, -1500                               # each codable, their difference is not
    with pytest.raises(ValueError):
        jpeg_craft.write([two], q, 8, 16, "gray")
    for bad in (np.zeros(64, np.uint16), np.full(64, 256, np.uint16)):
        with pytest.raises(ValueError):
            jpeg_craft.write(block(0, 1), bad, 8, 8, "gray")
    with pytest.raises(ValueError):
        jpeg_craft.write(block(0, 1), q, 8, 16, "gray")                # a block short


# ----------------------------------------------------------------------------- the rule on both sides
def test_constant_tables_patch_is_what_the_helper_says():
    for name, blob, p in jpeg_loud.loud()[::11]:
        q = jpeg_ref.parse(blob)
        assert np.array_equal(q["quant"], p["quant"]) and all(np.array_equal(a, b) for a, b in zip(q["coef"], p["coef"])), name


def test_loud_families_equal_pil_inside_the_rule_and_are_refused_outside(entropy):
    files = jpeg_loud.loud()
    assert len(files) == 24 * 3 + 8 * 3
    for name, _blob, p in files:
        ax, aw, lo, hi = jpeg_ref.ranges(p)
        if "-past-" not in name:
            band = int(name.rsplit("-v", 1)[1])
            # the largest constant inside the band: the next one is outside, and a step of the constant moves |v| by |v| / q
            assert max(-lo, hi) <= band and jpeg_ref.pinned(p), (name, ax, aw, lo, hi)
            assert max(-lo, hi) > band // 2, (name, lo, hi)
        else:
            past = {"v": lo < jpeg_ref.V_MIN or hi > jpeg_ref.V_MAX, "w": aw > jpeg_ref.W_LIMIT, "x": ax > jpeg_ref.X_LIMIT}
            assert past[name[-1]] and not jpeg_ref.pinned(p), (name, ax, aw, lo, hi)
    assert either_pil_or_refused(entropy, files) == (72, 24)
    # all four samplings reach the highest band, and at least one file CLAMPS there (v + 128 outside 0 .. 255)
    top = [p for name, _b, p in files if name.endswith("-v500")]
    assert {(p["components"], p["h"], p["v"]) for p in top} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert all(jpeg_ref.ranges(p)[3] > 127 or jpeg_ref.ranges(p)[2] < -128 for p in top)


def test_the_finding_every_file_now_equals_pil_or_is_refused(entropy):
    """The 288 files of the finding (constants that put max |coefficient * q| at 1, 0.5, 0.25 and 0.1 of 32767, all of which the
    rule `|coefficient * q| <= 32767` accepted): pinned ones equal PIL, every other one is refused."""
    pinned, refused = either_pil_or_refused(entropy, jpeg_loud.fractions())
    assert pinned + refused == 288 and pinned > 0 and refused > 160


def test_single_coefficients_up_to_the_last_pinned_amplitude(entropy):
    files = jpeg_loud.single()
    assert len(files) == 256
    for (name, _b, last), (_n, _b2, past) in zip(files[0::2], files[1::2]):
        k = int(name[7:9])
        assert name.endswith("last") and jpeg_ref.pinned(last) and not jpeg_ref.pinned(past)
        a, b = int(last["coef"][0][0, k]), int(past["coef"][0][0, k])
        assert abs(b) == abs(a) + 1 and a * b > 0 and np.count_nonzero(last["coef"][0]) == np.count_nonzero(past["coef"][0]) == 1
        lo, hi = jpeg_ref.ranges(last)[2:]
        assert max(-lo, hi) > 480, "%s stops at v in [%d, %d]: the search must end at the clamp's edge" % (name, lo, hi)
    assert either_pil_or_refused(entropy, files) == (128, 128)


def test_colour_clamp_at_every_corner(entropy):
    (name, blob, p), = jpeg_loud.corners()
    planes = [jpeg_ref.plane(p["coef"][c], p["quant"][c], 7, 49) for c in range(3)]
    seen = {(int(planes[0][8 * r, 8 * c]), int(planes[1][8 * r, 8 * c]), int(planes[2][8 * r, 8 * c])) for r in range(7) for c in range(49)}
    assert seen == {(y, cb, cr) for y in jpeg_loud.EDGE for cb in jpeg_loud.EDGE for cr in jpeg_loud.EDGE}
    assert all((pl.reshape(7, 8, 49, 8) == pl.reshape(7, 8, 49, 8)[:, :1, :, :1]).all() for pl in planes), "flat blocks"
    assert either_pil_or_refused(entropy, [(name, blob, p)]) == (1, 0)
    rgb = jpeg_ref.pixels(p)
    # by hand from the header: (0, 0, 0) -> G = (22554 * 128 + 46802 * 128 + 32768) >> 16 = 135; (255, 255, 255) -> 255 + ((-(22554 +
    # 46802) * 127 + 32768) >> 16) = 255 - 134
    assert rgb.min() == 0 and rgb.max() == 255 and (rgb[0, 0] == (0, 135, 0)).all() and (rgb[-1, -1] == (255, 121, 255)).all()


def test_upsampling_where_the_rounding_biases_decide(entropy):
    files = jpeg_loud.upsampling()
    assert len(files) == 2 * 36 * 2
    assert either_pil_or_refused(entropy, files) == (144, 0)
    # the files do sit where the biases decide: with the two biases exchanged the frame changes -- every "ramp" file that
    # interpolates (no replication), and every "flat" one with a block boundary inside the chroma plane in an interpolated direction
    checked = 0
    for name, _blob, p in files:
        boundary = p["width"] == 17 or (p["height"] == 17 and p["v"] == 2)
        if min(p["height"], p["width"]) >= 5 and (name.endswith("ramp") or boundary):
            assert not np.array_equal(_pixels_with_swapped_biases(p), jpeg_ref.pixels(p)), name
            checked += 1
    assert checked == 32 + 4 + 7


def _pixels_with_swapped_biases(p):
    """jpeg_ref.pixels with the upsampling's two biases exchanged (+ 2 / + 1 and + 7 / + 8): a wrong decoder."""
    H, W, h, v = p["height"], p["width"], p["h"], p["v"]
    y = jpeg_ref.plane(p["coef"][0], p["quant"][0], p["mcus_y"] * v, p["mcus_x"] * h)[:H, :W]
    n, m = -(-W // 2), -(-H // 2)
    chroma = []
    for c in (1, 2):
        s = jpeg_ref.plane(p["coef"][c], p["quant"][c], p["mcus_y"], p["mcus_x"]).astype(np.int64)
        if (h, v) == (2, 1):
            s = s[:H, :n]
            left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
            out = np.empty((H, 2 * n), np.int64)
            out[:, 0::2], out[:, 1::2] = (3 * s + left + 2) >> 2, (3 * s + right + 1) >> 2
        else:
            s = s[:m, :n]
            up, down = np.concatenate([s[:1], s[:-1]], 0), np.concatenate([s[1:], s[-1:]], 0)
            out = np.empty((2 * m, 2 * n), np.int64)
            for row, nb in ((0, up), (1, down)):
                t = 3 * s + nb
                left, right = np.concatenate([t[:, :1], t[:, :-1]], 1), np.concatenate([t[:, 1:], t[:, -1:]], 1)
                out[row::2, 0::2], out[row::2, 1::2] = (3 * t + left + 7) >> 4, (3 * t + right + 8) >> 4
        chroma.append(out[:H, :W])
    return jpeg_ref.colour(y, chroma[0], chroma[1])


# ----------------------------------------------------------------------------- the screen
def test_blocks_inside_the_block_sum_screen_hold_every_limb():
    """csrc/jpeg_host.cpp runs the exact passes only on a block with S = sum |x| > SCREEN_SUM.  Blocks with S at the limit and
    just under it -- one loud value at each position, values on every position with the signs that add up at one sample, seeded
    random sparse and dense ones -- hold all three limbs, by ranges()' exact integers."""
    text = open(os.path.join(ROOT, "single-shot-detector_amd", "csrc", "jpeg_host.cpp")).read()
    S = int(re.search(r"constexpr int SCREEN_SUM = (\d+);", text).group(1))
    assert S == 2047
    limits = [int(re.search(r"\b%s = (-?\d+)" % n, text).group(1)) for n in ("X_LIMIT", "W_LIMIT", "V_MIN", "V_MAX")]
    assert limits == [jpeg_ref.X_LIMIT, jpeg_ref.W_LIMIT, jpeg_ref.V_MIN, jpeg_ref.V_MAX]
    rng = np.random.default_rng(2047)
    blocks = []
    for k in range(64):                                             # everything on one position
        for sign in (1, -1):
            b = np.zeros(64, np.int64)
            b[k] = sign * S
            blocks.append(b)
    basis = np.stack([np.outer(np.cos((2 * (s // 8) + 1) * np.arange(8) * np.pi / 16), np.cos((2 * (s % 8) + 1) * np.arange(8) * np.pi / 16)).reshape(64)
                      for s in range(64)])                          # [sample, position]: the sign each position has at a sample
    for s in range(64):
        for sign in (1, -1):
            for spread in (64, 8, 3):                               # the positions of the largest gain at this sample
                order = np.argsort(-np.abs(basis[s]))[:spread]
                b = np.zeros(64, np.int64)
                b[order] = S // spread
                b[order[0]] += S - int(b.sum())
                blocks.append(sign * np.where(basis[s] < 0, -b, b))
    for _ in range(3000):
        count = int(rng.choice([1, 2, 3, 5, 8, 16, 40, 64]))
        at = rng.choice(64, count, replace=False)
        total = S - int(rng.integers(0, 4))                          # at the limit and just under it
        cuts = np.sort(rng.integers(0, total + 1, count - 1))
        mags = np.diff(np.concatenate([[0], cuts, [total]]))
        b = np.zeros(64, np.int64)
        b[at] = mags * rng.choice([-1, 1], count)
        blocks.append(b)
    blocks = np.stack(blocks)
    sums = np.abs(blocks).sum(1)
    assert len(blocks) > 3000 and sums.max() == S and sums.min() >= S - 3
    ax, aw, lo, hi = jpeg_ref.block_ranges(blocks, np.ones(64, np.int64))
    # the bounds of the derivation in csrc/jpeg_host.cpp, which lie inside the limbs
    assert ax.max() <= S and aw.max() < 11359 and lo.min() > -495 and hi.max() < 495
    assert jpeg_ref.blocks_pinned(blocks, np.ones(64, np.int64)).all()
