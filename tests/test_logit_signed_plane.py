"""No GPU: the class-logit screen's signed weight plane (pack_screen of csrc/weights.hip) and the integer operand selects of
logit_screen_kernel (screen_operand), restated in numpy by helpers/logit_signed_plane.py on the roundings of
helpers/logit_screen_ref.py.  The P wave and the N wave must take out of one 16-bit word exactly the operands the two
planes held before: otherwise the bound U of DESIGN 4.2 is not the one that was proven."""
import numpy as np

from helpers import logit_signed_plane as sp


def same_f16(bits, values):
    """uint16 words against float16 values: the same bits, any NaN for a NaN."""
    got = np.asarray(bits, np.uint16).view(np.float16)
    want = np.asarray(values, np.float16)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan])


def test_selects_on_every_half_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wp, wn = sp.decode(bits)
    p, n = sp.select_p(bits), sp.select_n(bits)
    assert same_f16(p, wp)
    assert same_f16(n, wn)
    # the selects give +0 or the magnitude, never a set sign; at most one of the two is non-zero
    assert not (p & 0x8000).any() and not (n & 0x8000).any()
    assert not ((p != 0) & (n != 0)).any()
    # a NaN with its sign clear stays that NaN in P; -0 (never packed) would be +0 in both
    assert p[0x7e00] == 0x7e00 and n[0x7e00] == 0
    assert p[0x8000] == 0 and n[0x8000] == 0
    assert p[0xfbff] == 0 and n[0xfbff] == 0x7bff


SPECIAL = np.array([0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -15, -2.0 ** -15, 1e-7, -1e-7, 2.0 ** -14 * (1 - 2.0 ** -12),
                    -2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -14 * (1 + 2.0 ** -12), -2.0 ** -14 * (1 + 2.0 ** -12),
                    np.float32(1e-45), -np.float32(1e-45), 65504.0, -65504.0, 65505.0, -65505.0, 65520.0, -65520.0, 7e4, -7e4,
                    3.0e38, -3.0e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.1, -0.1], np.float32)


def test_round_trip_of_special_and_random_weights():
    rng = np.random.default_rng(3)
    w = np.concatenate([SPECIAL,
                        rng.standard_normal(20000).astype(np.float32) * np.float32(0.05),
                        (rng.standard_normal(20000) * 10.0 ** rng.uniform(-9, 6, 20000)).astype(np.float32),
                        np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)])
    bits = sp.encode(w)
    wp, wn = sp.operands(w)
    assert same_f16(sp.select_p(bits), wp.astype(np.float16))
    assert same_f16(sp.select_n(bits), wn.astype(np.float16))
    assert not (bits == 0x8000).any(), "a weight encodes to -0"
    by = {float(v): int(b) for v, b in zip(SPECIAL, sp.encode(SPECIAL)) if v == v}
    assert by[0.0] == 0 and sp.encode(np.float32([-0.0]))[0] == 0
    assert by[2.0 ** -14] == 0x0400 and by[-2.0 ** -14] == 0x8400
    assert by[2.0 ** -15] == 0x0400 and by[-2.0 ** -15] == 0            # up to the smallest normal / down to nothing
    assert by[float(np.float32(1e-7))] == 0x0400 and by[float(np.float32(-1e-7))] == 0
    assert by[65504.0] == 0x7bff and by[-65504.0] == 0xfbff
    assert by[65505.0] == 0x7c00 and by[-65505.0] == 0xfbff             # just beyond: up to inf / down to 65504
    assert by[np.inf] == 0x7c00 and by[-np.inf] == 0xfbff
    assert sp.encode(np.float32([np.nan]))[0] & 0xfc00 == 0x7c00 and sp.encode(np.float32([np.nan]))[0] & 0x03ff
