"""The COCO accumulation without a GPU (include/ssd_hip.h, "the COCO accumulation"): the flat-array restatement
(tests/helpers/coco_accumulate_ref.py) equals CocoBoxEval.accumulate() bit for bit through both packings; the order of pack_order
against the per-category mergesort; the c_r rule against np.searchsorted; the header's constants; the entry point's refusals, which
come before any HIP call; and the host path, unchanged."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import coco_accumulate_cases as acases
from helpers import coco_accumulate_ref as aref
from helpers import coco_match_cases as cases
from helpers import coco_match_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = tuple(cases.SEEDS) + ("hand",)


def make(name):
    return acases.hand_built() if name == "hand" else cases.make(name)


@pytest.fixture(scope="module")
def sets(ssd):
    """name -> (annotations, results, the host's CocoBoxEval evaluated and accumulated)"""
    out = {}
    for name in SETS:
        gt, dets = make(name)
        out[name] = (gt, dets, ssd.coco_metric.CocoBoxEval(gt, dets).evaluate().accumulate())
    return out


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def restated(ssd, q, matched, ignored, gt_ignore):
    metric = ssd.coco_metric
    return aref.accumulate(q["segments"], q["order"], q["rank"], matched, ignored, gt_ignore, len(metric.IOU_THRS), metric.MAX_DETS, metric.REC_THRS)


def test_python_constants_are_the_headers(ssd):
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    ca, metric = ssd.coco_accumulate, ssd.coco_metric
    assert (ca.MAX_MAXDETS, ca.MAX_REC, ca.MAX_THR, ca.MAX_AREA, ca.MAX_DET, ca.CELLS_PER_BLOCK, ca.GRID_CAP) == tuple(
        value("SSD_COCO_" + n) for n in ("MAX_MAXDETS", "MAX_REC", "MAX_THR", "MAX_AREA", "MAX_DET", "CELLS_PER_BLOCK", "GRID_CAP"))
    assert len(metric.MAX_DETS) <= ca.MAX_MAXDETS and len(metric.REC_THRS) <= ca.MAX_REC and len(metric.IOU_THRS) <= ca.MAX_THR
    # the struct: four int64 fields in the header's order, 32 bytes, no padding
    body = re.search(r"typedef struct ssd_coco_segment \{(.*?)\} ssd_coco_segment;", hdr, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == list(ca.SEGMENT_DTYPE.names) == ["det_begin", "det_count", "gt_begin", "gt_count"]
    assert "32 bytes, no padding" in re.search(r"typedef struct ssd_coco_segment \{[^\n]*", hdr).group(0)
    assert ca.SEGMENT_DTYPE.itemsize == 32 and all(ca.SEGMENT_DTYPE.fields[n][0] == np.dtype("<i8") for n in fields)
    assert [ca.SEGMENT_DTYPE.fields[n][1] for n in fields] == [0, 8, 16, 24]


@pytest.mark.parametrize("name", SETS)
def test_restatement_equals_accumulate_through_pack_cells(ssd, sets, name):
    """host evaluate() -> cells() -> pack_cells -> the restatement: the upload route's arrays"""
    gt, dets, host = sets[name]
    q = ssd.coco_accumulate.pack_cells(host.cells(), host.cat_ids, host.img_ids, len(ssd.coco_metric.AREA_RNG))
    precision, recall = restated(ssd, q, q["matched"], q["ignored"], q["gt_ignore"])
    assert same_bits(precision, host.precision) and same_bits(recall, host.recall)
    assert (precision > 0).any() and (precision == 0).any() and ((precision == -1).any() or name != "hand")


@pytest.mark.parametrize("name", SETS)
def test_restatement_equals_accumulate_through_pack_order(ssd, sets, name):
    """coco_match.pack -> the matching's restatement -> pack_order -> the restatement: the retained route's arrays"""
    gt, dets, host = sets[name]
    metric = ssd.coco_metric
    p = ssd.coco_match.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    assert p["packed"].all()
    m, i, g = mref.match(p["cells"], p["det_box"], p["det_area"], p["gt_box"], p["gt_area"], p["gt_crowd"], metric.THR_L, metric.AREA_RNG)
    q = ssd.coco_accumulate.pack_order(p, host.cat_ids)
    precision, recall = restated(ssd, q, m, i, g)
    assert same_bits(precision, host.precision) and same_bits(recall, host.recall)
    # ... and the two packings are the same arrays
    u = ssd.coco_accumulate.pack_cells(host.cells(), host.cat_ids, host.img_ids, len(metric.AREA_RNG))
    for key in ("order", "rank", "segments"):
        assert q[key].dtype == u[key].dtype and np.array_equal(q[key], u[key]), key
    assert np.array_equal(m, u["matched"]) and np.array_equal(i, u["ignored"]) and np.array_equal(g, u["gt_ignore"])


def test_the_hand_built_set_holds_every_shape(ssd, sets):
    """What tests/helpers/coco_accumulate_cases.py promises, read off the packed arrays and the host's result."""
    gt, dets, host = sets["hand"]
    metric, ca = ssd.coco_metric, ssd.coco_accumulate
    q = ca.pack_cells(host.cells(), host.cat_ids, host.img_ids, len(metric.AREA_RNG))
    seg = q["segments"]
    k = lambda cat: host.cat_ids.index(cat)
    assert [int(seg["det_count"][k(c)]) for c in (11, 12, 13, 14, 15, 16)] == [1, 63, 64, 65, 128, 129]
    assert seg["det_count"][k(1)] == 0 and seg["gt_count"][k(1)] == 5                       # groundtruth, no detection: n = 0
    assert (host.recall[:, k(1), 0, :] == 0).all() and (host.precision[:, :, k(1), 0, :] == 0).all()
    assert seg["det_count"][k(2)] == 5 and seg["gt_count"][k(2)] == 0 and (host.precision[:, :, k(2)] == -1).all()
    assert seg["det_count"][k(acases.EMPTY_CATEGORY)] == 0 and seg["gt_count"][k(acases.EMPTY_CATEGORY)] == 0
    assert (host.recall[:, k(3), 2:] == -1).all() and (host.recall[:, k(3), :2] >= 0).all()  # all boxes small
    assert seg["det_count"][k(5)] == 107 and q["rank"].max() == 99                          # 130 truncated to 100, + 7
    npig = lambda cat: int(np.count_nonzero(q["gt_ignore"][0, seg["gt_begin"][k(cat)]:seg["gt_begin"][k(cat)] + seg["gt_count"][k(cat)]] == 0))
    assert [npig(c) for c in (7, 8, 9, 10)] == [1, 3, 100, 150]
    # ties inside a cell and across images: the order's third key decides
    score = host.cells()["scores"]
    assert len(set(score.tolist())) < len(score) / 10
    # ignored rows lead category 6 at 'all': 0 / eps, then a true positive
    rows = q["order"][seg["det_begin"][k(6)]:][:4]
    assert (q["ignored"][0, rows] & 1).all() and host.recall[0, k(6), 0, 2] > 0
    # a category that never reaches recall 1: zeros at the tail of the precision row
    r9 = host.recall[0, k(9), 0, 2]
    assert 0 < r9 < 1 and host.precision[0, -1, k(9), 0, 2] == 0 and host.precision[0, 0, k(9), 0, 2] > 0
    # maxDets 1 and 10 take the first 1 / 10 of every cell: fewer rows than maxDets 100
    assert host.recall[0, k(5), 0, 0] <= host.recall[0, k(5), 0, 1] <= host.recall[0, k(5), 0, 2]


@pytest.mark.parametrize("name", SETS)
def test_pack_order_is_the_per_category_mergesort(ssd, sets, name):
    gt, dets, host = sets[name]
    ca = ssd.coco_accumulate
    p = ssd.coco_match.pack(host._gts, host._dts, host.cat_ids, host.img_ids)
    q = ca.pack_order(p, host.cat_ids)
    cells, score = p["cells"], p["det_score"]
    assert q["order"].dtype == np.int32 and q["rank"].dtype == np.uint8 and q["segments"].dtype == ca.SEGMENT_DTYPE
    assert q["nd"] == len(score) == len(q["order"]) and q["ng"] == len(p["gt_area"])
    assert np.array_equal(q["rank"], np.concatenate([np.arange(d) for d in cells["D"]] + [np.zeros(0, np.int64)]).astype(np.uint8))
    d_end = g_end = 0
    for k, cat in enumerate(host.cat_ids):
        mine = [n for n, (c, _img) in enumerate(p["keys"]) if c == cat]
        seg = q["segments"][k]
        assert seg["det_begin"] == d_end and seg["gt_begin"] == g_end
        assert seg["det_count"] == cells["D"][mine].sum() and seg["gt_count"] == cells["G"][mine].sum()
        a, b = d_end, d_end + int(seg["det_count"])
        want = a + np.argsort(-score[a:b], kind="mergesort")               # the category's rows are [a, b) of the packed arrays
        assert np.array_equal(q["order"][a:b], want)
        d_end, g_end = b, g_end + int(seg["gt_count"])
    assert d_end == q["nd"] and g_end == q["ng"]


@pytest.mark.parametrize("npig", [1, 2, 3, 7, 100, 101, 1000])
def test_first_count_is_searchsorted_over_every_recall(ssd, npig):
    """c_r against np.searchsorted over the recalls of all counts 0 .. npig, for the 101 thresholds; at npig = 100 c / 100 and the
    linspace value differ in the last bit for some c: the exact test decides, not the estimate."""
    thr = ssd.coco_metric.REC_THRS
    rc = np.arange(npig + 1, dtype=np.float64) / np.float64(npig)
    want = np.searchsorted(rc, thr, side="left")
    got = np.array([aref.first_count(x, npig) for x in thr])
    assert np.array_equal(got, want) and got[0] == 0 and got[-1] == npig
    if npig == 100:
        assert (rc != thr).any()                               # the case the exact test is for
    # ... and beyond the thresholds of a real run: below 0, and above 1, where only counts past npig would do
    for x, c in ((-0.5, 0), (0.0, 0), (1.0000000000000002, npig + 1), (7.0, 7 * npig), (1e300, 2 ** 31)):
        assert aref.first_count(x, npig) == c
    more = np.linspace(-0.1, 2.0, 211)
    assert np.array_equal([aref.first_count(x, npig) for x in more], np.searchsorted(np.arange(2 * npig + 2, dtype=np.float64) / np.float64(npig), more))


def test_the_entry_point_refuses_before_any_hip_call(ssd):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the call
    never reads."""
    lib, ca, metric = ssd.lib(), ssd.coco_accumulate, ssd.coco_metric
    nd, ng = 6, 5
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    rec = np.array(metric.REC_THRS, np.float64)
    dets = np.array(metric.MAX_DETS, np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    good = np.zeros(2, ca.SEGMENT_DTYPE)
    good["det_begin"], good["det_count"], good["gt_begin"], good["gt_count"] = [0, 4], [4, 2], [0, 2], [2, 3]

    def call(segments=good, K=None, T=10, A=4, M=len(dets), R=len(rec), nd=nd, ng=ng, **kw):
        a = dict(segments_host=segments.ctypes.data, segments_dev=fake, order=fake, rank=fake, matched=fake, ignored=fake, gt_ignore=fake,
                 max_dets=dets.ctypes.data_as(ip), rec_thr=rec.ctypes.data_as(dp), rec_thr_dev=fake, precision=fake, recall=fake)
        a.update(kw)
        rc = lib.ssd_coco_accumulate(a["segments_host"], a["segments_dev"], len(segments) if K is None else K, a["order"], a["rank"],
                                     a["matched"], a["ignored"], nd, a["gt_ignore"], ng, T, A, a["max_dets"], M, a["rec_thr"],
                                     a["rec_thr_dev"], R, a["precision"], a["recall"], None)
        return rc, lib.ssd_last_error().decode()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("ssd_coco_accumulate: ") and word in msg, (rc, msg)

    for name, arg in (("segments_host", "segments_host"), ("segments_dev", "segments_dev"), ("order", "order_dev"), ("rank", "rank_dev"),
                      ("matched", "matched_dev"), ("ignored", "ignored_dev"), ("gt_ignore", "gt_ignore_dev"), ("max_dets", "max_dets_host"),
                      ("rec_thr", "rec_thr_host"), ("rec_thr_dev", "rec_thr_dev"), ("precision", "precision_dev"), ("recall", "recall_dev")):
        refused(arg + " is NULL", **{name: None})
    for name, arg, n in (("segments_dev", "segments_dev", 8), ("order", "order_dev", 4), ("matched", "matched_dev", 2), ("ignored", "ignored_dev", 2),
                         ("rec_thr_dev", "rec_thr_dev", 8), ("precision", "precision_dev", 8), ("recall", "recall_dev", 8)):
        refused("%s must be %d-byte aligned" % (arg, n), **{name: fake + n // 2})
    wide_d, wide_i = np.arange(256, dtype=np.float64), np.arange(1, 257, dtype=np.int32)
    refused("T must be in [1, 16]", T=0)
    refused("T must be in [1, 16]", T=17)
    refused("A must be in [1, 4]", A=0)
    refused("A must be in [1, 4]", A=5)
    refused("M must be in [1, 4]", M=0)
    refused("M must be in [1, 4]", M=5, max_dets=wide_i.ctypes.data_as(ip))
    refused("R must be in [1, 128]", R=0)
    refused("R must be in [1, 128]", R=129, rec_thr=wide_d.ctypes.data_as(dp))
    refused("K must be in [0, 2^20]", K=-1)
    refused("K must be in [0, 2^20]", K=(1 << 20) + 1)
    refused("nd must be in [0, 2^31 - 1]", nd=-1)
    refused("nd must be in [0, 2^31 - 1]", nd=1 << 31)
    refused("ng must be in [0, 2^40]", ng=-1)
    refused("ng must be in [0, 2^40]", ng=(1 << 40) + 1)
    for bad, at in (([0, 10, 100], 0), ([-1, 10, 100], 0), ([1, 1, 100], 1), ([1, 10, 9], 2)):
        refused("max_dets_host[%d] must be positive and above" % at, max_dets=np.array(bad, np.int32).ctypes.data_as(ip))
    for value, at in ((np.nan, 3), (np.inf, 100), (-np.inf, 0)):
        r = rec.copy()
        r[at] = value
        refused("rec_thr_host[%d] must be finite" % at, rec_thr=r.ctypes.data_as(dp))
    r = rec.copy()
    r[50] = r[48]
    refused("rec_thr_host[50] must be finite and not below", rec_thr=r.ctypes.data_as(dp))

    def segments(**kw):
        s = good.copy()
        for k, v in kw.items():
            s[k] = v
        return s
    refused("segment 1: det_count must not be negative", segments=segments(det_count=[4, -1]))
    refused("segment 0: gt_count must not be negative", segments=segments(gt_count=[-2, 3]))
    refused("segment 0: det_begin must be the end of the segment before", segments=segments(det_begin=[1, 4]))
    refused("segment 1: det_begin must be the end of the segment before", segments=segments(det_begin=[0, 3]))
    refused("segment 1: det_begin must be the end of the segment before", segments=segments(det_begin=[0, 5]))
    refused("segment 1: det_begin + det_count runs past nd", segments=segments(det_count=[4, 3]))
    refused("the segments' detection ranges end at 5, not at nd", segments=segments(det_count=[4, 1]))
    refused("segment 1: gt_begin overlaps", segments=segments(gt_begin=[0, 1]))
    refused("segment 0: gt_begin overlaps", segments=segments(gt_begin=[-1, 2]))
    refused("segment 1: gt_begin + gt_count runs past ng", segments=segments(gt_begin=[0, 3]))
    # what is NOT refused returns 0 without a launch: K == 0, with every array NULL
    rc, msg = call(segments=good[:0], nd=0, ng=0, segments_host=None, segments_dev=None, order=None, rank=None, matched=None, ignored=None,
                   gt_ignore=None, rec_thr_dev=None, precision=None, recall=None)
    assert rc == 0, msg


def test_pack_cells_refuses_half_a_cell(ssd, sets):
    gt, dets, host = sets[0]
    cells = host.cells()
    keep = np.ones(len(cells["D"]), bool)
    keep[int(np.nonzero(cells["keys"][:, 1] == 2)[0][3])] = False              # one (category, image) loses its 'medium' cell
    half = ssd.coco_metric.CocoBoxEval(gt, dets)
    half.eval_imgs = {tuple(k): host.eval_imgs[tuple(k)] for k, ok in zip(cells["keys"].tolist(), keep) if ok}
    with pytest.raises(ValueError, match="area range 2 holds other cells"):
        ssd.coco_accumulate.pack_cells(half.cells(), half.cat_ids, half.img_ids, 4)


@pytest.mark.parametrize("name", SETS)
def test_the_host_path_is_unchanged(ssd, sets, name):
    """accumulate() and accumulate(device=None) are the loops they were: the same arrays as the module-level evaluate_boxes."""
    gt, dets, host = sets[name]
    ev = ssd.coco_metric.CocoBoxEval(gt, dets).evaluate(unpack=False)            # (unpack without a device: the host loop, eval_imgs built)
    assert isinstance(ev.__dict__["eval_imgs"], dict) and list(ev.eval_imgs) == list(host.eval_imgs)
    ev.accumulate(device=None)
    assert same_bits(ev.precision, host.precision) and same_bits(ev.recall, host.recall)
    assert np.array_equal(ev.summarize(), ssd.coco_metric.evaluate_boxes(gt, dets))
