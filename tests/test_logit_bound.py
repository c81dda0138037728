"""The screen's bound (csrc/logit_screen.hip) restated in numpy, without a GPU:

    xu  = x rounded UP to a normal f16 (0 stays 0, a positive value below 2^-14 becomes 2^-14, past 65504: inf)
    Wp  = max(w, 0) rounded up to a normal f16;  Wn = max(-w, 0) rounded DOWN, a subnormal result flushed to 0
    P^  = sum xu * Wp,  N^ = sum xu * Wn   in ANY order, every add off by a relative u' = 2^-22 at most (the matrix pipe)
    cst = bias + 2^-14 sum Wn + 2^-20 |bias|, rounded up to fp32
    U   = ((P^ (1 + 2^-9) - N^ (1 - 2^-9)) + cst) + 2^-18 ((P^ + N^) + |cst|)         in fp32

U must never fall below the fp32 logit: acc = fmaf(x_k, w_k, acc) from +0 over k ascending, then acc + bias.  The directed
f16 roundings are emulated in float64 (exact: a float64 holds every f16 and every fp32 product of two of them), the fmaf
chain in float64 rounded to fp32 per step (a product of two fp32 values is exact in float64; the one double rounding of the
sum is covered by the chain's own error term many times over).  This pins 2^-9, 2^-18 and the constant independently of
the GPU."""
import numpy as np

from helpers.logit_screen_ref import E_PIPE, K, U_PIPE, envelope, f16_down, f16_up, screen_constant


def fmaf_chain(x, w, bias):
    """[n, K] fp32 operands -> the fp32 logits of the k-ascending fmaf chain from +0, plus the bias."""
    acc = np.zeros(x.shape[0], np.float32)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(x.shape[1]):
            acc = (x64[:, k] * w64[:, k] + acc.astype(np.float64)).astype(np.float32)
        return (acc + bias.astype(np.float32)).astype(np.float32)


def perturbed_sum(terms, rng):
    """Sum of non-negative terms [n, K] in a random order, every partial sum multiplied by 1 + e, |e| <= u' -- once with
    random signs, once always down (the worst case for P^) and once always up (the worst case for N^)."""
    n, k = terms.shape
    order = rng.permutation(k)
    t = terms[:, order]
    outs = []
    for mode in (0, -1, 1):
        s = np.zeros(n, np.float64)
        for j in range(k):
            e = rng.uniform(-U_PIPE, U_PIPE, n) if mode == 0 else mode * U_PIPE
            s = (s + t[:, j]) * (1.0 + e)
        outs.append(s)
    return outs          # random, low, high


def bounds(x, w, bias, rng):
    """U per perturbation tried (fp32, per row): [random errors, P as low and N as high as the pipe may make them]."""
    xu = f16_up(x.astype(np.float64))
    wp = f16_up(np.maximum(w, 0).astype(np.float64))
    wn = f16_down(np.maximum(-w, 0).astype(np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        P = perturbed_sum(xu * wp, rng)
        N = perturbed_sum(xu * wn, rng)
        b = bias.astype(np.float64)
        c = b + np.ldexp(wn.sum(axis=1) * (1.0 + 1e-9), -14) + np.ldexp(np.abs(b), -20) + 1e-30
        cst = c.astype(np.float32)
        cst = np.where(cst.astype(np.float64) < c, np.nextafter(cst, np.float32(np.inf)), cst).astype(np.float32)
        out = []
        for Ph, Nh in ((P[0], N[0]), (P[1], N[2]), (P[2], N[1])):       # the third: P high, N low -- the largest U the pipe may give
            Pf, Nf = Ph.astype(np.float32), Nh.astype(np.float32)
            t1 = (Pf * np.float32(1.001953125)).astype(np.float32)
            t2 = (Nf * np.float32(0.998046875)).astype(np.float32)
            u = ((t1 - t2).astype(np.float32) + cst).astype(np.float32)
            u = (u + (np.float32(2.0 ** -18) * ((Pf + Nf).astype(np.float32) + np.abs(cst)).astype(np.float32)).astype(np.float32)).astype(np.float32)
            out.append(u)
    return out


def bound(x, w, bias, rng):
    """The smallest U over the first two perturbations (fp32), per row."""
    worst = None
    for u in bounds(x, w, bias, rng)[:2]:
        worst = u if worst is None else np.where(np.isnan(u) | np.isnan(worst), np.float32(np.nan), np.minimum(u, worst))
    return worst


def draws(rng, n, kind, K=K):
    w = rng.normal(0.0, 0.01 * np.sqrt(2304.0 / K), (n, K)).astype(np.float32)
    x = np.maximum(rng.normal(0.5, 2.0, (n, K)), 0).astype(np.float32)
    bias = rng.uniform(-8.0, -1.0, n).astype(np.float32)
    if kind == "overflow":
        x = (x * np.float32(3e4)).astype(np.float32)             # part of the activations past 65504
    elif kind == "subnormal":
        x = rng.uniform(0.0, 2.0 ** -14, (n, K)).astype(np.float32)
        bias = rng.uniform(-2.0, -1.5, n).astype(np.float32)
    elif kind == "zero":
        x = np.zeros((n, K), np.float32)
    elif kind == "negative":
        w = -np.abs(w)
    elif kind == "positive":
        w = np.abs(w)
    elif kind == "tiny_w":
        w = (w * np.float32(1e-4)).astype(np.float32)            # weights that are subnormal halves
    elif kind == "mixed_scale":
        x = (x * np.exp(rng.uniform(-12, 6, (n, K)))).astype(np.float32)
        w = (w * np.exp(rng.uniform(-6, 6, (n, K)))).astype(np.float32)
    elif kind == "cancel":                                       # P and N large and nearly equal
        w = (w * np.float32(30.0)).astype(np.float32)
        bias = np.zeros(n, np.float32)
    return x, w, bias


def test_bound_never_below_the_fp32_chain():
    rng = np.random.default_rng(2304)
    kinds = ["plain"] * 4 + ["overflow", "subnormal", "zero", "negative", "positive", "tiny_w", "mixed_scale", "cancel"]
    total, margin = 0, []
    # every kind at the logits convolution's own K = 2304, and eight times as many draws of each on a short chain
    for kind, n, k in [(kd, 1000, K) for kd in kinds] + [(kd, 8000, 72) for kd in kinds]:
        x, w, bias = draws(rng, n, kind, k)
        L = fmaf_chain(x, w, bias)
        U = bound(x, w, bias, rng)
        # the kernel marks unless U < lo: a NaN or inf U marks, so only an ordered U below the logit is a failure
        with np.errstate(invalid="ignore"):
            bad = U < L
        assert not bad.any(), (kind, k, int(bad.sum()), float((L - U)[bad].max()))
        ok = np.isfinite(U) & np.isfinite(L)
        if ok.any():
            margin.append(("%s K=%d" % (kind, k), float((U - L)[ok].min()), float(np.median((U - L)[ok]))))
        total += n
    assert total >= 100000
    for m in margin:
        print("%-20s slack U - L: min %.3g median %.3g" % m)


def test_directed_roundings_bracket_their_operand():
    rng = np.random.default_rng(7)
    v = np.abs(rng.normal(0, 1, 20000) * np.exp(rng.uniform(-30, 12, 20000)))
    up, dn = f16_up(v), f16_down(v)
    assert (up >= v).all() and (dn <= v).all()
    assert ((up == 0) | (up >= 2.0 ** -14)).all() and ((dn == 0) | (dn >= 2.0 ** -14)).all()
    norm = (v >= 2.0 ** -14) & (v <= 65504)
    assert (up[norm] <= v[norm] * (1 + 2.0 ** -10)).all() and (dn[norm] >= v[norm] * (1 - 2.0 ** -10)).all()
    assert f16_up(np.array([0.0]))[0] == 0.0 and np.isinf(f16_up(np.array([65505.0]))[0])


def test_envelope_is_never_below_the_screen_bound_and_not_vacuous():
    """helpers/logit_screen_ref.py: U_hi, from the exact sums alone, is at or above U for every perturbed summation order
    (the pipe's errors random, against the bound, and for it), and it still leaves octets unmarked."""
    rng = np.random.default_rng(950)
    lo = np.float32(np.log(0.15 / 0.85) - 1e-3 * (1.0 + abs(np.log(0.15 / 0.85))))      # conservative_logit_bound(0.15) of csrc/plan.hip
    kinds = ["plain", "overflow", "subnormal", "zero", "negative", "positive", "tiny_w", "mixed_scale", "cancel"]
    marked = {}
    for kind, n, k in [(kd, 400, K) for kd in kinds] + [(kd, 4000, 72) for kd in kinds]:
        x, w, bias = draws(rng, n, kind, k)
        xu = f16_up(x.astype(np.float64))
        wp = f16_up(np.maximum(w, 0).astype(np.float64))
        wn = f16_down(np.maximum(-w, 0).astype(np.float64))
        with np.errstate(over="ignore", invalid="ignore"):
            hi = envelope((xu * wp).sum(axis=1), (xu * wn).sum(axis=1), screen_constant(wn.sum(axis=1), bias))
            for which, U in enumerate(bounds(x, w, bias, rng)):
                bad = hi < U
                assert not bad.any(), (kind, k, which, int(bad.sum()), float((U - hi)[bad].max()))
            may = ~(hi < lo)
        octs = may.reshape(-1, 8).any(axis=1)           # 8 consecutive draws as the 8 columns of an octet
        marked[(kind, k)] = (int(octs.sum()), octs.size)
        print("%-12s K=%-4d envelope marks %d of %d octets" % ((kind, k) + marked[(kind, k)]))
    assert E_PIPE == K * U_PIPE
    for key in (("plain", K), ("plain", 72)):
        assert 0 < marked[key][0] < marked[key][1], (key, marked[key])
    assert sum(m for m, _ in marked.values()) < sum(t for _, t in marked.values())
