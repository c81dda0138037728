"""tests/helpers/guarded.py on CPU tensors: the three layouts' residues, no unguarded byte between tensors of odd sizes, check() on
an untouched arena, and one planted byte reported with its tensor, side and offset -- the proof that the GPU tests of
tests/test_gpu_train_guards.py can fail."""
import numpy as np
import pytest
import torch

from helpers.guarded import GUARD, LAYOUTS, SENTINEL, Arena, GuardError, Separate

f32 = np.float32


def _arena(layout, sizes=((2, 1, 1, 33), (4,), (40,))):
    """Inputs x (contract 16), bias (4), frames (uint8, 4); outputs out (16), dbias (4), dw (16), stat (16); a workspace (16)."""
    rng = np.random.default_rng(3)
    a = Arena(torch, "cpu", layout)
    a.add("x", rng.normal(0, 1, sizes[0]).astype(f32), f32, 16, "input")
    a.add("bias", rng.normal(0, 1, sizes[1]).astype(f32), f32, 4, "input")
    a.add("frames", rng.integers(0, 256, 37).astype(np.uint8), np.uint8, 4, "input")
    a.add("out", sizes[0], f32, 16, "output")
    a.add("dbias", sizes[1], f32, 4, "output", fill=-7.5)
    a.add("one", (1,), np.uint8, 4, "output", fill=9)
    a.add("dw", sizes[2], f32, 16, "output")
    a.add("stat", (5, 20), f32, 16, "output")
    a.add("labels", (7,), np.int32, 4, "output")
    a.add("four", (1,), f32, 4, "output")
    a.add("ws", (1000,), np.uint8, 16, "workspace")
    return a


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_give_the_stated_residues(layout):
    a = _arena(layout)
    t = a.tensors
    assert a.view("x").data_ptr() - a.offset("x") == a.dev.data_ptr() and a.dev.data_ptr() % 512 == 0
    c16 = [n for n in t if t[n].contract == 16]
    c4 = [n for n in t if t[n].contract == 4]
    assert c16 == ["x", "out", "dw", "stat", "ws"] and c4 == ["bias", "frames", "dbias", "one", "labels", "four"]
    if layout == "aligned":
        assert all(a.offset(n) % 512 == 0 for n in t)
        return
    if layout == "mixed":
        assert a.offset("x") % 512 == 0                       # the first input; the others move up one place
        c16 = c16[1:]
    assert [a.offset(n) % 256 for n in c16] == [16 * o for o in (1, 3, 5, 7, 9)[:len(c16)]]
    assert all(a.offset(n) % 32 == 16 for n in c16)           # 16-byte aligned and never 32
    assert [a.offset(n) % 16 for n in c4] == [4, 8, 12, 4, 8, 12]
    for n in t:
        assert a.view(n).data_ptr() % t[n].contract == 0 and a.ptr(n) == a.view(n).data_ptr()


def test_the_odd_residues_cycle_through_all_eight():
    a = Arena(torch, "cpu", "skewed")
    for i in range(10):
        a.add("t%d" % i, (4,), f32, 16, "output")
    assert [a.offset("t%d" % i) % 256 // 16 for i in range(10)] == [1, 3, 5, 7, 9, 11, 13, 15, 1, 3]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_byte_between_tensors_is_a_guard_byte(layout):
    """264, 4 and 1 byte tensors (no multiples of 16): the mask is True exactly outside the writable tensors, at least GUARD
    bytes lie in front of and behind every tensor, and the guard holds the sentinel WORD from the tensor's last byte + 1."""
    a = _arena(layout)
    a.view("x")
    t = sorted(a.tensors.values(), key=lambda v: v.start)
    assert {v.nbytes for v in t} >= {264, 4, 1, 16, 37}
    covered = np.zeros(len(a.host), bool)
    for v in t:
        covered[v.start:v.start + v.nbytes] = True
    writable = np.zeros(len(a.host), bool)
    for v in t:
        if v.role != "input":
            writable[v.start:v.start + v.nbytes] = True
    assert np.array_equal(a.mask, ~writable)
    assert t[0].start >= GUARD and len(a.host) - (t[-1].start + t[-1].nbytes) >= GUARD + 512
    for u, v in zip(t, t[1:]):
        assert v.start - (u.start + u.nbytes) >= 2 * GUARD
    words = np.resize(np.frombuffer(SENTINEL.tobytes(), np.uint8), len(a.host))
    assert np.array_equal(a.host[~covered], words[~covered])
    got = a.dev.numpy()
    assert np.array_equal(got, a.host)
    out = a.tensors["out"]
    assert not covered[out.start + 264] and covered[out.start + 263]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_check_passes_on_an_untouched_arena_and_after_writing_every_output(layout):
    a = _arena(layout)
    a.check()
    for n, v in a.tensors.items():
        if v.role != "input":
            a.view(n).fill_(1)
    a.check()
    assert np.isnan(_arena(layout).read("out")).all() and (_arena(layout).read("dbias") == f32(-7.5)).all()
    assert (_arena(layout).read("ws") == 0xFF).all() and (_arena(layout).read("labels") == 0x7FC00000).all()
    x = np.random.default_rng(3).normal(0, 1, (2, 1, 1, 33)).astype(f32)
    assert np.array_equal(a.read("x"), x) and a.view("x").is_contiguous() and tuple(a.view("x").shape) == (2, 1, 1, 33)
    assert a.view(None) is None and a.ptr(None) is None
    assert set(a.outputs()) == {"out", "dbias", "one", "dw", "stat", "labels", "four"}


PLANTED = [("out", +264, "out", "back", 1), ("out", -1, "out", "front", 1), ("ws", 1000 - 1 + 1023, "ws", "back", 1023),
           ("x", 17, "x", "inside", 17), ("one", 1, "one", "back", 1), ("dbias", -GUARD, "dbias", "front", GUARD),
           ("bias", 16 + GUARD - 1, "bias", "back", GUARD)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tensor,at,name,side,offset", PLANTED, ids=["%s%+d" % (p[0], p[1]) for p in PLANTED])
def test_one_planted_byte_is_reported_with_name_side_and_offset(layout, tensor, at, name, side, offset):
    """One byte written with torch at `at` bytes from the tensor's first byte: 1 byte behind an output, 1 byte in front of it,
    1023 bytes behind a workspace, inside an input, behind a 1-byte tensor, and the two ends of a guard."""
    a = _arena(layout)
    p = a.offset(tensor) + at
    a.dev[p] = int(a.host[p]) ^ 0x01
    with pytest.raises(GuardError) as e:
        a.check()
    assert (e.value.name, e.value.side, e.value.offset) == (name, side, offset), str(e.value)
    assert e.value.from_end == at - (a.tensors[tensor].nbytes - 1)            # signed, from the tensor's last byte
    assert "'%s'" % name in str(e.value) and isinstance(e.value, AssertionError)
    a.dev[p] = int(a.host[p])
    a.check()


def test_the_first_changed_byte_is_reported_and_the_count():
    a = _arena("skewed")
    o = a.offset("dw")
    a.dev[o + 160 + 4:o + 160 + 20] = 0
    with pytest.raises(GuardError, match="16 bytes changed.*5 bytes behind the end of 'dw'"):
        a.check()


def test_a_write_of_the_sentinels_own_bytes_inside_an_input_is_still_seen():
    a = _arena("mixed")
    a.view("bias").view(torch.int32)[2] = int(np.int32(np.uint32(SENTINEL).view(np.int32)))
    with pytest.raises(GuardError) as e:
        a.check()
    assert (e.value.name, e.value.side) == ("bias", "inside") and 8 <= e.value.offset < 12


def test_the_control_has_the_same_interface():
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (3, 6)).astype(f32)
    m = Separate(torch, "cpu")
    m.add("x", x, f32, 16, "input")
    m.add("y", (3, 6), f32, 16, "output")
    m.add("mm", (8,), f32, 16, "output", fill=np.arange(8, dtype=f32))
    m.add("ws", (0,), np.uint8, 16, "workspace")
    assert np.array_equal(m.read("x"), x) and np.isnan(m.read("y")).all() and np.array_equal(m.read("mm"), np.arange(8, dtype=f32))
    assert m.view("ws").numel() == 0 and m.view(None) is None
    m.check()
    m.view("x")[0, 0] += 1
    with pytest.raises(AssertionError, match="'x'"):
        m.check()
    with pytest.raises(RuntimeError):
        m.add("late", (1,), f32, 16, "output")


def test_add_refuses_what_the_layout_cannot_mean():
    a = Arena(torch, "cpu", "skewed")
    a.add("x", np.zeros(4, f32), f32, 16, "input")
    for bad in (dict(name="x", array_or_shape=(4,), dtype=f32, contract=16, role="output"),          # a name twice
                dict(name="y", array_or_shape=(4,), dtype=f32, contract=8, role="output"),
                dict(name="y", array_or_shape=(4,), dtype=f32, contract=16, role="scratch"),
                dict(name="y", array_or_shape=(4,), dtype=f32, contract=16, role="input"),           # an input without content
                dict(name="y", array_or_shape=np.zeros(4, f32), dtype=f32, contract=16, role="output"),
                dict(name="y", array_or_shape=(4,), dtype=f32, contract=16, role="workspace")):
        with pytest.raises(ValueError):
            a.add(**bad)
    with pytest.raises(ValueError):
        Arena(torch, "cpu", "packed")
