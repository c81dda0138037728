"""The TRAIN step's norms without a GPU: the numpy restatement against math.fsum of the exact squares, its tree and its block order on
hand-made cases where the order of the additions decides the last bit, and every refusal of ssd_train_norms and its planner through
the loaded library (all of them come before any HIP call)."""
import ctypes
import math

import numpy as np
import pytest

from helpers import train_norms_ref as ref

f32 = np.float32
BIG = f32(2.0 ** 27)                    # its square, 2^54, has an ulp of 4: adding 1 is lost, adding 2 is a tie, adding 4 is exact
P54 = 2.0 ** 54


@pytest.mark.parametrize("n,pad", [(1, 0), (5, 3), (4096, 0), (4097, 1), (3 * 4096 + 5, 2), (20000, 3)])
def test_restatement_is_within_n_half_ulps_of_the_exact_sum(n, pad):
    rng = np.random.default_rng(n + pad)
    x = (rng.normal(0, 1, n) * np.exp2(rng.integers(-40, 41, n))).astype(f32)
    got, bad = ref.tensor_norm(x, pad)
    exact = math.fsum(float(v) * float(v) for v in x)                # each product is exact in double, fsum adds them exactly
    rel = abs(float(got) - exact) / exact
    print("n %d pad %d: relative error %.3g (bound %.3g)" % (n, pad, rel, n * 2.0 ** -53))
    assert bad == 0 and rel <= n * 2.0 ** -53


def test_non_finite_elements_count_and_add_nothing():
    x = np.arange(1, 11, dtype=f32)
    want = float((x.astype(np.float64) ** 2).sum())
    y = x.copy()
    y[[0, 4, 9]] = [np.nan, np.inf, -np.inf]
    got, bad = ref.tensor_norm(y, 1)
    assert bad == 3 and float(got) == want - 1.0 - 25.0 - 100.0
    assert ref.tensor_norm(np.zeros(0, f32), 0) == (0.0, 0) and ref.tensor_norm(np.zeros(0, f32), 3) == (0.0, 0)
    sums, bads = ref.table_norms([(x, None, 0), (x, y, 2)])
    assert sums.tolist() == [[want, 0.0], [want, want - 126.0]] and bads.tolist() == [[0, 0], [0, 3]]


def _at(n, items, pad=0):
    x = np.zeros(n, f32)
    for virtual, value in items:
        x[virtual - pad] = value
    return x


def test_a_lane_adds_its_own_elements_first_and_in_order():
    # lane 0 owns virtual elements 0..3 (k = 0): 2^54 + 1 + 1 + 1 loses every 1; lane 1 owns 4..7: 1 + 1 + 1 + 1 = 4, and the tree
    # adds 4 to 2^54 exactly.  A plain left-to-right sum gives 2^54, the correctly rounded sum 2^54 + 8.
    x = _at(8, [(0, BIG)] + [(j, 1) for j in range(1, 8)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54 + 4
    # k = 1 of lane 0 is virtual element 1024: still lane 0's own running sum, so these four are lost as well
    x = _at(1028, [(0, BIG)] + [(1024 + e, 1) for e in range(4)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54
    # the same values seen from a tensor that starts 3 floats into its 16-byte group: element 0 is virtual element 3, alone in lane
    # 0's quad; elements 1..4 fill lane 1's quad
    x = _at(5, [(3, BIG)] + [(j, 1) for j in range(4, 8)], pad=3)
    assert float(ref.tensor_norm(x, 3)[0]) == P54 + 4


def test_the_tree_is_a_t_plus_a_t_plus_s_from_128_down():
    lane = lambda t: 4 * t                                            # the first virtual element of lane t (k = 0)
    # lanes 0, 64 and 128: s = 128 adds lane 128's 2 to lane 0 (a tie: 2^54 stays), s = 64 adds lane 64's 2 (a tie again)
    x = _at(4096, [(lane(0), BIG), (lane(64), 1), (lane(64) + 1, 1), (lane(128), 1), (lane(128) + 1, 1)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54
    # lanes 0, 64 and 192: s = 128 makes lane 64 hold 2 + 2 = 4, which s = 64 adds to 2^54 exactly
    x = _at(4096, [(lane(0), BIG), (lane(64), 1), (lane(64) + 1, 1), (lane(192), 1), (lane(192) + 1, 1)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54 + 4
    # lanes 0, 1, 2, 3: s = 2 gives a[0] = 2^54 + 2 = 2^54 (tie) and a[1] = 2 + 2 = 4; s = 1 adds 4 exactly.  Adjacent pairs first
    # ((a0 + a1) + (a2 + a3)) would give the same here, a sequential sum 2^54
    x = _at(4096, [(0, BIG)] + [(lane(t) + e, 1) for t in (1, 2, 3) for e in (0, 1)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54 + 4


def test_blocks_are_added_in_ascending_order():
    # partials 2, 2^54, 2: (0 + 2) + 2^54 is a tie and rounds to 2^54 (even), + 2 is a tie again: 2^54.  Any order that meets the
    # two 2s first gives 2^54 + 4
    x = _at(3 * 4096, [(0, 1), (4, 1), (4096, BIG), (2 * 4096, 1), (2 * 4096 + 4, 1)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54
    # partials 2^54, 2, 2: both ties round down as well; 2, 2, 2^54: 4 + 2^54 is exact
    x = _at(3 * 4096, [(0, BIG), (4096, 1), (4100, 1), (2 * 4096, 1), (2 * 4096 + 4, 1)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54
    x = _at(3 * 4096, [(0, 1), (4, 1), (4096, 1), (4100, 1), (2 * 4096, BIG)])
    assert float(ref.tensor_norm(x, 0)[0]) == P54 + 4


# ----------------------------------------------------------------------------- the refusals
def _rows(train_step):
    rows = np.zeros(3, train_step.TENSOR_DTYPE)
    for c in ("w", "grad", "m", "v", "ema"):
        rows[c] = 0x10000                       # never dereferenced: every refusal comes before any HIP call
    rows["count"] = (5000, 10, 4096)
    rows["decay"] = (1, 0, 0)
    rows["first_block"] = (0, 2, 3)
    return rows


def test_both_entry_points_refuse_what_the_update_refuses_and_the_planner_returns_zero(ssd):
    from ssd_amd import train_step
    L = ssd.lib()
    rows = _rows(train_step)
    fake = ctypes.c_void_p(0x20000)
    out = ctypes.c_void_p(0x30000)
    NEED = 4 * 32                               # 2 + 1 + 1 blocks

    def plan(r=rows, T=3):
        return L.ssd_train_norms_workspace_bytes(r.ctypes.data_as(ctypes.c_void_p) if r is not None else None, T)

    def call(r=rows, dev=fake, T=3, sums=out, bad=out, ws=fake, nbytes=NEED):
        return L.ssd_train_norms(r.ctypes.data_as(ctypes.c_void_p) if r is not None else None, dev, T, sums, bad, ws, nbytes, None)
    assert plan() == NEED == 32 * train_step.block_starts(rows["w"], rows["count"])[1]
    for kw in ({"r": None}, {"dev": None}, {"T": 0}, {"T": -1}, {"T": 65537}, {"dev": ctypes.c_void_p(0x20004)}):
        assert call(**kw) == -1, kw
        assert L.ssd_last_error().decode().startswith("ssd_train_norms:"), kw
        if "dev" not in kw:
            assert plan(**kw) == 0, kw
    for field, value, word in (("count", -1, "count"), ("count", (1 << 40) + 1, "count"), ("w", 0, "NULL"), ("m", 0, "NULL"),
                               ("v", 0, "NULL"), ("ema", 0, "NULL"), ("w", 0x10002, "aligned"), ("m", 0x10001, "aligned"),
                               ("v", 0x10003, "aligned"), ("ema", 0x10002, "aligned"), ("grad", 0x10002, "aligned"),
                               ("decay", 2, "decay"), ("first_block", 1, "first_block")):
        q = rows.copy()
        q[1][field] = value
        assert call(r=q) == -1, field
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_train_norms:") and "tensor 1" in msg and word in msg, (field, msg)
        assert plan(r=q) == 0, field
        assert L.ssd_last_error().decode().startswith("ssd_train_norms_workspace_bytes:")
    # more than 2^31 - 1 blocks: 2^40 elements are 2^28 blocks a row
    many = np.zeros(9, train_step.TENSOR_DTYPE)
    for c in ("w", "m", "v", "ema"):
        many[c] = 0x10000
    many["count"] = 1 << 40
    many["first_block"][:8] = np.arange(8, dtype=np.int64) << 28
    assert call(r=many, T=9) == -1 and "2^31 - 1 blocks" in L.ssd_last_error().decode()
    assert plan(r=many, T=9) == 0
    # the update's block rule: 2 + 4094 elements are one block, so tensor 1 would start at block 1
    q = rows.copy()
    q[0]["w"], q[0]["count"] = 0x10008, 4094
    assert call(r=q) == -1 and "tensor 1: first_block must be 1" in L.ssd_last_error().decode() and plan(r=q) == 0
    q[0]["count"] = 4095
    assert plan(r=q) == NEED
    # a NULL grad is no refusal, and a table of empty tensors needs no workspace bytes
    q = rows.copy()
    q["grad"] = 0
    assert plan(r=q) == NEED
    q["count"], q["first_block"] = 0, 0
    assert plan(r=q) == 0


def test_outputs_and_workspace_are_refused_before_any_hip_call(ssd):
    from ssd_amd import train_step
    L = ssd.lib()
    rows = _rows(train_step)
    p = rows.ctypes.data_as(ctypes.c_void_p)
    fake, out = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    for sums, bad, ws, nbytes, word in ((None, out, fake, 128, "NULL sums or bad"), (out, None, fake, 128, "NULL sums or bad"),
                                        (ctypes.c_void_p(0x30004), out, fake, 128, "8-byte aligned"),
                                        (out, ctypes.c_void_p(0x30004), fake, 128, "8-byte aligned"),
                                        (out, out, None, 128, "NULL workspace"),
                                        (out, out, ctypes.c_void_p(0x20008), 128, "16-byte aligned"),
                                        (out, out, fake, 127, "too small"), (out, out, fake, 0, "too small")):
        assert L.ssd_train_norms(p, fake, 3, sums, bad, ws, nbytes, None) == -1, word
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_train_norms:") and word in msg, (word, msg)


def test_the_call_layer_checks_its_tensors_on_the_cpu(ssd):
    import torch
    from ssd_amd import train_calls, train_step
    rows = torch.from_numpy(_rows(train_step).view(np.uint8).copy())
    assert train_calls.train_norms_workspace_bytes(rows) == 128 == train_calls.train_norms_workspace_bytes(rows, 3)
    with pytest.raises(ValueError, match="rows_host"):
        train_calls.train_norms_workspace_bytes(rows[:100])
    with pytest.raises(ValueError, match="exactly T"):
        train_calls.train_norms_workspace_bytes(rows, 2)
    sums, bad = torch.zeros((3, 2), dtype=torch.float64), torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="rows_dev"):
        train_calls.train_norms(rows, rows[:56], sums, bad)
    with pytest.raises(ValueError, match="sums"):
        train_calls.train_norms(rows, rows, sums.float(), bad)
    with pytest.raises(ValueError, match="bad"):
        train_calls.train_norms(rows, rows, sums, bad[:2])
    with pytest.raises(TypeError, match="GPU"):
        train_calls.train_norms(rows, rows, sums, bad)
