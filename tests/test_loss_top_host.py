"""The per-level top losses without a GPU (include/ssd_hip.h, "the per-level top losses"): the count rule against the
reference's float32 expression, the numpy restatement (helpers/loss_top_ref.py) against what is order-free in the reference, every
refusal of the three entry points by its text and before any HIP call, the header against the binding and the call layer, and
differentiable_loss's default signature."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from helpers import loss_top_ref as ref

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_LEVELS = (38400, 9600, 2400, 600, 150)           # 640 x 640: six anchors on 80^2, 40^2, 20^2, 10^2, 5^2 cells


def _i64(values):
    return (ctypes.c_int64 * max(len(values), 1))(*values)


# ----------------------------------------------------------------------------- the count rule
def test_the_count_rule_is_the_references_float32_expression_up_to_2_pow_20():
    n = np.arange(1, (1 << 20) + 1, dtype=np.int64)
    assert np.array_equal((n + 4) // 5, ref.reference_count(n))
    assert ref.counts(TRAIN_LEVELS) == [7680, 1920, 480, 120, 30] == list(ref.reference_count(np.array(TRAIN_LEVELS)))


def test_the_library_counts_by_the_same_rule(ssd):
    from ssd_amd import train_calls
    assert train_calls.loss_top_counts(TRAIN_LEVELS) == (7680, 1920, 480, 120, 30)
    for levels in ((1,), (5,), (6,), (150, 37, 5, 1, 1), (163840,), (163836, 4, 3, 2, 1, 1, 1, 1), tuple(range(1, 9))):
        assert list(train_calls.loss_top_counts(levels)) == ref.counts(levels), levels
        assert train_calls.loss_top_workspace_bytes(3, levels) == 2 * 3 * sum(ref.counts(levels)) * 4, levels


# ----------------------------------------------------------------------------- the restatement
def test_the_keys_order_every_bit_pattern_as_the_header_says():
    bits = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800001, 0xFF800000, 0xFF7FFFFF, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000,
                     0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7F800001, 0x7FC00000,
                     0x7FFFFFFF], u32)           # -NaN .. -inf, -FLT_MAX .. -denormal, -0.0, +0.0, denormals .. +inf, +NaN
    k = ref.keys(bits.view(f32))
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(ref.values(k).view(u32), bits)
    rng = np.random.default_rng(0)
    any_bits = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(u32)
    assert np.array_equal(ref.values(ref.keys(any_bits.view(f32))).view(u32), any_bits)
    finite = any_bits.view(f32)[np.isfinite(any_bits.view(f32))]
    order = np.argsort(ref.keys(finite), kind="stable")
    assert np.all(np.diff(finite[order].astype(np.float64)) >= 0)     # the key order is the value order where values are ordered


@pytest.mark.parametrize("levels", [(150, 37, 5, 1, 1), (23,), (6, 5, 4)])
def test_at_batch_one_the_means_are_the_largest_k_of_every_level(levels):
    rng = np.random.default_rng(sum(levels))
    pool = rng.standard_normal(40).astype(f32)                         # ties everywhere, also across rank k
    planes = pool[rng.integers(0, 40, (2, 1, sum(levels)))]
    M = ref.means(planes, levels)
    V = ref.selected(planes, levels)
    assert np.array_equal(M.view(u32), V[:, 0].view(u32))              # (0.0 + x) / 1 keeps every bit of a finite x
    off = koff = 0
    for n, k in zip(levels, ref.counts(levels)):
        for p in range(2):
            seg = planes[p, 0, off:off + n]
            want = np.sort(np.partition(seg, n - k)[n - k:])           # the reference's set, order-free
            assert np.array_equal(np.sort(M[p, koff:koff + k]), want)
            assert np.all(np.diff(M[p, koff:koff + k]) <= 0)           # ... in this library's order
        off, koff = off + n, koff + k


def test_the_mean_is_one_double_sum_rounded_once_and_one_division():
    V = np.array([[[1.0], [2.0 ** -24], [2.0 ** -24]], [[3.0], [5.0], [-8.0]]], f32)       # [2, B = 3, N = 1]
    M = ref.means(V, (1,))
    assert M[0, 0] == f32(1.0 + 2.0 ** -23) / f32(3)                   # a float32 chain loses both half-ulp terms to ties-to-even
    assert M[0, 0] != (f32(1.0) + f32(2.0 ** -24) + f32(2.0 ** -24)) / f32(3)
    assert M[1, 0] == f32(0.0) and not np.signbit(M[1, 0])
    zeros = np.full((2, 2, 1), -0.0, f32)
    assert not np.signbit(ref.means(zeros, (1,))).any()                # the sum starts at +0.0


def test_minus_zero_sorts_below_plus_zero_and_the_tail_is_the_threshold():
    seg = np.array([0.0, -0.0, 0.0, 2.0, -0.0, 0.0, 0.0, -1.0, 0.0, 0.0], f32)
    got = ref.top(seg, 8)
    assert np.array_equal(got.view(u32), np.array([2.0] + [0.0] * 6 + [-0.0], f32).view(u32))


# ----------------------------------------------------------------------------- the refusals
def test_every_refusal_comes_with_its_text_before_any_hip_call(ssd):
    L = ssd.lib()
    levels, N = (150, 37, 5, 1, 1), 194
    K = sum(ref.counts(levels))
    planes, means, ws = ctypes.c_void_p(0x10004), ctypes.c_void_p(0x20004), ctypes.c_void_p(0x30010)   # never dereferenced
    NEED = 2 * 3 * K * 4

    def call(cls=planes, loc=planes, B=3, N=N, lv=levels, n_levels=None, means=means, ws=ws, nbytes=NEED, null_levels=False):
        return L.ssd_loss_top_means(cls, loc, B, N, None if null_levels else _i64(lv), len(lv) if n_levels is None else n_levels, means, ws,
                                    nbytes, None)
    for kw, word in (({"cls": None}, "NULL cls_losses_dev"), ({"loc": None}, "NULL cls_losses_dev"), ({"means": None}, "NULL cls_losses_dev"),
                     ({"cls": ctypes.c_void_p(0x10002)}, "4-byte aligned"), ({"loc": ctypes.c_void_p(0x10001)}, "4-byte aligned"),
                     ({"means": ctypes.c_void_p(0x20006)}, "4-byte aligned"),
                     ({"B": 0}, "B must be at least 1"), ({"B": -2}, "B must be at least 1"),
                     ({"null_levels": True}, "NULL anchors_per_level"),
                     ({"n_levels": 0}, "n_levels must be in [1, 8]"), ({"lv": (1,) * 9, "N": 9}, "n_levels must be in [1, 8]"),
                     ({"lv": (150, 0, 42, 1, 1)}, "anchors_per_level[1] must be at least 1"),
                     ({"lv": (150, 37, -5, 1, 1)}, "anchors_per_level[2] must be at least 1"),
                     ({"N": 195}, "sum to 194 anchors, N is 195"),
                     ({"lv": (1 << 24,), "N": 1 << 24}, "below 2^24"), ({"lv": ((1 << 23), (1 << 23)), "N": 1 << 24}, "below 2^24"),
                     ({"lv": (163841,), "N": 163841}, "above SSD_LOSS_TOP_MAX_K = 32768"),
                     ({"ws": None}, "NULL workspace"), ({"ws": ctypes.c_void_p(0x30008)}, "16-byte aligned"),
                     ({"nbytes": NEED - 1}, "workspace too small"), ({"nbytes": 0}, "workspace too small")):
        assert call(**kw) == -1, kw
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_loss_top_means:") and word in msg, (kw, msg)
    # the planner returns 0 and the counts -1 for the same levels
    out = _i64((0,) * 9)
    for lv, n_levels, word in (((150, 0, 42), 3, "at least 1"), ((1,) * 9, 9, "n_levels"), ((1,), 0, "n_levels"), ((1 << 24,), 1, "2^24"),
                               ((163841,), 1, "SSD_LOSS_TOP_MAX_K")):
        assert L.ssd_loss_top_workspace_bytes(3, _i64(lv), n_levels) == 0, lv
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_loss_top_workspace_bytes:") and word in msg, msg
        assert L.ssd_loss_top_counts(_i64(lv), n_levels, out) == -1, lv
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_loss_top_counts:") and word in msg, msg
    assert L.ssd_loss_top_workspace_bytes(0, _i64(levels), 5) == 0 and "B must be at least 1" in L.ssd_last_error().decode()
    assert L.ssd_loss_top_workspace_bytes(3, None, 5) == 0 and "NULL anchors_per_level" in L.ssd_last_error().decode()
    assert L.ssd_loss_top_counts(_i64(levels), 5, None) == -1 and "NULL k_out" in L.ssd_last_error().decode()
    assert L.ssd_loss_top_counts(None, 5, out) == -1 and "NULL anchors_per_level" in L.ssd_last_error().decode()
    # the largest level a call takes: k = SSD_LOSS_TOP_MAX_K exactly
    assert L.ssd_loss_top_counts(_i64((163840,)), 1, out) == 32768 == out[0]
    assert L.ssd_loss_top_workspace_bytes(3, _i64(levels), 5) == NEED


def test_the_call_layer_checks_its_tensors_on_the_cpu(ssd):
    import torch
    from ssd_amd import train_calls
    levels = (150, 37, 5, 1, 1)
    K = sum(ref.counts(levels))
    cls, loc, means = torch.zeros((3, 194)), torch.zeros((3, 194)), torch.zeros((2, K))
    with pytest.raises(ValueError, match="cls_losses"):
        train_calls.loss_top_means(cls.double(), loc, levels, means)
    with pytest.raises(ValueError, match="loc_losses"):
        train_calls.loss_top_means(cls, loc[:2], levels, means)
    with pytest.raises(ValueError, match="means"):
        train_calls.loss_top_means(cls, loc, levels, means[:, :-1].contiguous())
    with pytest.raises(ValueError, match="anchors_per_level"):
        train_calls.loss_top_counts(5)
    with pytest.raises(ssd.SsdError, match="at least 1"):
        train_calls.loss_top_counts((150, 0))
    with pytest.raises(TypeError, match="GPU"):
        train_calls.loss_top_means(cls, loc, levels, means)


# ----------------------------------------------------------------------------- header, binding, signatures
def test_the_header_the_binding_and_the_call_layer_agree(ssd):
    from ssd_amd import _lib, train_calls
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert int(re.search(r"#define SSD_LOSS_TOP_MAX_K (\d+)", hdr).group(1)) == train_calls.LOSS_TOP_MAX_K == 32768
    assert int(re.search(r"#define SSD_LOSS_MAX_LEVELS (\d+)", hdr).group(1)) == train_calls.LOSS_MAX_LEVELS
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    kinds = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
             "void *": ctypes.c_void_p, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
    for name, res in (("ssd_loss_top_counts", ctypes.c_int64), ("ssd_loss_top_workspace_bytes", ctypes.c_size_t),
                      ("ssd_loss_top_means", ctypes.c_int)):
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert {"int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "int": ctypes.c_int}[m.group(1)] is res is _lib.SIGNATURES[name][0]
        args = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in m.group(2).split(",")]
        assert [kinds[a] for a in args] == _lib.SIGNATURES[name][1], (name, args)
    assert "loss_top.hip" in _lib._SOURCES
    # the capacity the header states: the sort buffer and the bins fit one workgroup's 160 KiB
    assert 4 * train_calls.LOSS_TOP_MAX_K + 4 * (256 + 8) <= 160 * 1024 and 5 * train_calls.LOSS_TOP_MAX_K == 163840


def test_differentiable_loss_and_train_keep_their_defaults(ssd, capsys):
    sig = inspect.signature(ssd.differentiable_loss)
    assert list(sig.parameters) == ["class_predictions", "encoded_boxes", "anchors", "groundtruth", "params", "anchors_per_level", "per_image",
                                    "per_anchor"]
    assert sig.parameters["per_image"].default is False and sig.parameters["per_anchor"].default is False
    assert sig.parameters["anchors_per_level"].default == ()
    for fn in (ssd.Trainer.train, ssd.Trainer.train_and_evaluate):
        p = inspect.signature(fn).parameters
        assert p["loss_histograms"].default is False and list(p)[-1] == "loss_histograms" and p["save_summary_steps"].default == 0
    from ssd_amd import train
    with pytest.raises(SystemExit):
        train.main(["--help"])
    assert "--loss-histograms" in capsys.readouterr().out
