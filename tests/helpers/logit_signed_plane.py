"""The screen's ONE signed weight plane (pack_screen of csrc/weights.hip, screen_operand of csrc/logit_screen.hip) restated in
numpy, no GPU.  The directed roundings are those of helpers/logit_screen_ref.py (f16_up, f16_down); this file adds only how
the two operands share a 16-bit word:

    bits of Wp             where w > 0 or w is NaN      (sign clear)
    0x8000 | bits of Wn    where Wn is non-zero         (sign set)
    +0                     everywhere else              (never -0)

decode() is the definition of (Wp, Wn) from a word of the plane; select_p / select_n are the integer operations the kernel's
P wave and N wave apply to the 16-bit halves."""
import numpy as np

from helpers import logit_screen_ref as ref


def operands(w):
    """float array of weights -> (Wp, Wn) as float64, the way logit_screen_ref.upper_bound forms them: Wp = f16_up(max(w, 0)),
    Wn = f16_down(max(-w, 0)), a NaN weight -> Wp = NaN, Wn = 0."""
    with np.errstate(invalid="ignore"):         # (signalling NaN patterns among the inputs)
        w = np.asarray(w, np.float64)
    nanw = np.isnan(w)
    z = np.where(nanw, 0.0, w)
    wp = ref.f16_up(np.maximum(z, 0.0))
    wn = ref.f16_down(np.maximum(-z, 0.0))
    wp[nanw] = np.nan
    return wp, wn


def encode(w):
    """float array of weights -> the plane's uint16 words."""
    wp, wn = operands(w)
    with np.errstate(over="ignore"):
        pb = wp.astype(np.float16).view(np.uint16)
        nb = wn.astype(np.float16).view(np.uint16)
    assert not (np.nan_to_num(wp) != 0).__and__(wn != 0).any(), "Wp and Wn both non-zero"
    return np.where(nb != 0, nb | np.uint16(0x8000), pb).astype(np.uint16)


def decode(bits):
    """uint16 words -> (Wp, Wn) as float16 VALUES: the word itself where its sign is clear, minus the word where it is set."""
    bits = np.asarray(bits, np.uint16)
    neg = (bits & 0x8000) != 0
    mag = (bits & np.uint16(0x7fff)).astype(np.uint16).view(np.float16)
    zero = np.float16(0.0)
    return np.where(neg, zero, mag), np.where(neg, mag, zero)


def select_p(bits):
    """The P wave: signed 16-bit max with 0."""
    return np.maximum(np.asarray(bits, np.uint16).view(np.int16), np.int16(0)).view(np.uint16)


def select_n(bits):
    """The N wave: flip the sign bit, then signed 16-bit max with 0."""
    return np.maximum((np.asarray(bits, np.uint16) ^ np.uint16(0x8000)).view(np.int16), np.int16(0)).view(np.uint16)
