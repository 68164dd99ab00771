"""Accuracy pin of include/mog_math.h (the framework's definition of its fp32
elementary functions), on the CPU oracle's compilation of it.

The deterministic input set of tests/math_spec_cases.py -- every exponent x
64 mantissas x both signs, the specials, +-2 ulps around every branch constant
of the header, a 400 001-point linspace over [-110, 90] and the worst inputs
earlier sweeps recorded -- goes through oracle_math_vec and is compared with
float64 numpy in ulps of the float32-rounded reference (floored at 2^-149).

The bound per function is the maximum this sweep measured, rounded up to the
next quarter ulp (measured: exp 0.862 at -71.0325, log 1.677 at 1.281, expm1
2.671 at 0.4, tanh 2.397 at -0.2105, sigmoid 2.156 at -16.6535, softplus 2.029
at 0.23736973, log1p 3.243 at 0.029860657).  They bound this set, not every
float: an exhaustive scan of [2^-6, 2^-4) finds log1p at 3.79 ulp
(x = 0.030236896).  The same bounds stand in the header comment of mog_math.h.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from math_spec_cases import (  # noqa: E402
    EXP, EXP_HI, EXPM1, FLT_MIN, LOG, LOG1P, NAMES, SIGMOID, SOFTPLUS, SOFTPLUS_T, TANH, TANH_SAT,
    oracle_math, same_bits, spec_inputs)

# ulps; include/mog_math.h quotes these
BOUND = {EXP: 1.0, LOG: 1.75, EXPM1: 2.75, TANH: 2.5, SIGMOID: 2.25, SOFTPLUS: 2.25, LOG1P: 3.25}

# sigmoid is exactly 1 from here on (1 + exp(-x) rounds to 1), and exactly 0
# from -EXP_HI down (exp(-x) is +inf: above the threshold by the test in
# mog_expf, at the threshold through its polynomial), where the true value is
# a subnormal near 2.9e-39
SIGMOID_ONE = np.float32(16.63553237915039)

REF = {EXP: np.exp, LOG: np.log, EXPM1: np.expm1, TANH: np.tanh,
       SIGMOID: lambda v: 1.0 / (1.0 + np.exp(-v)), SOFTPLUS: lambda v: np.logaddexp(0.0, v),
       LOG1P: np.log1p}


@pytest.fixture(scope="module")
def xs():
    x = spec_inputs()
    return x[np.isfinite(x)]


def _domain(fn, x):
    if fn == LOG:
        return x[x > 0]
    if fn == LOG1P:
        return x[x > -1]
    if fn == SIGMOID:
        return x[x > -EXP_HI]  # exactly 0 from there down: test_sigmoid_saturation
    if fn == SOFTPLUS:
        return x[x >= 0]  # x < 0: test_softplus_branches
    return x


def _ulp_err(got, ref64):
    ref32 = ref64.astype(np.float32)
    # the gap above |ref32| (np.spacing, which overflows at FLT_MAX's binade)
    ulp = np.maximum(np.ldexp(1.0, np.frexp(np.abs(ref32).astype(np.float64))[1] - 24), 2.0 ** -149)
    return np.abs(got.astype(np.float64) - ref64) / ulp


@pytest.mark.parametrize("fn", sorted(BOUND))
def test_ulp_bound_on_the_pinned_set(fn, xs):
    x = _domain(fn, xs)
    got = oracle_math(fn, x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # float64 exp overflows to inf on purpose
        ref = REF[fn](x.astype(np.float64))
        ref32 = ref.astype(np.float32)
    # where the float32-rounded reference overflows, so does the spec
    over = ~np.isfinite(ref32)
    np.testing.assert_array_equal(got[over], ref32[over])
    err = _ulp_err(got[~over], ref[~over])
    i = int(np.argmax(err))
    print(f"{NAMES[fn]}: max {err[i]:.4f} ulp at x = {x[~over][i]!r}, bound {BOUND[fn]}")
    assert err[i] <= BOUND[fn], (NAMES[fn], float(err[i]), float(x[~over][i]))
    # the bound is the measured maximum rounded up to the next quarter ulp
    assert err[i] > BOUND[fn] - 0.25, (NAMES[fn], float(err[i]))


def test_specials():
    """NaN, +-inf and +-0 through every function.  expm1 and tanh return +0
    for -0 (x + x^2 p with an fma; the sign applied only where x < 0)."""
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    x = np.array([nan, inf, -inf, 0.0, -0.0], f)
    want = {EXP: [nan, inf, 0, 1, 1], LOG: [nan, inf, nan, -inf, -inf], EXPM1: [nan, inf, -1, 0, 0],
            TANH: [nan, 1, -1, 0, 0], SIGMOID: [nan, 1, 0, 0.5, 0.5],
            SOFTPLUS: [nan, inf, 0, np.log(f(2)), np.log(f(2))], LOG1P: [nan, inf, nan, 0, -0.0]}
    for fn, w in want.items():
        got = oracle_math(fn, x)
        w = np.array(w, f)
        if fn == SOFTPLUS:  # log(2) through mog_logf: within its bound, not a known bit pattern
            assert abs(float(got[3]) - np.log(2.0)) <= BOUND[LOG] * 2.0 ** -24 and got[3] == got[4]
            got, w = got[:3], w[:3]
        assert same_bits(got, w).all(), (NAMES[fn], got, w)


def test_sigmoid_saturation(xs):
    y = oracle_math(SIGMOID, xs)
    assert np.all(y[xs <= -EXP_HI] == 0) and np.all(y[xs > -EXP_HI] > 0)
    assert np.all(y[xs >= SIGMOID_ONE] == 1) and np.all(y[xs < SIGMOID_ONE] < 1)
    edge = np.array([-EXP_HI, np.nextafter(-EXP_HI, np.float32(0)),
                     np.nextafter(SIGMOID_ONE, np.float32(0)), SIGMOID_ONE], np.float32)
    ye = oracle_math(SIGMOID, edge)
    assert ye[0] == 0 and 0 < ye[1] < FLT_MIN  # a subnormal, 2.9e-39
    assert ye[2] == np.float32(1 - 2.0 ** -23) and ye[3] == 1  # 1 / (1 + 2^-23)
    assert np.all(np.diff(oracle_math(SIGMOID, np.sort(xs))) >= 0)


def test_tanh_saturation(xs):
    y = oracle_math(TANH, xs)
    big = np.abs(xs) > TANH_SAT
    np.testing.assert_array_equal(y[big], np.sign(xs[big]))
    assert np.all(np.abs(y) <= 1)
    # odd, bit for bit (the sign is applied last), but for tanh(-0) = +0
    nz = xs != 0
    assert same_bits(oracle_math(TANH, -xs[nz]), -y[nz]).all()


def test_softplus_branches(xs):
    """TF-1.12 Softplus: x above 13.94..., exp(x) below -13.94..., and
    log(exp(x) + 1) evaluated in fp32 between.  Near the low threshold
    exp(x) + 1 keeps few bits of exp(x): that cancellation is the reference's,
    so x < 0 is held to an absolute error (the rounding of exp(x) + 1, 2^-24,
    plus mog_logf's 1.75 ulps of a result below ln 2: under 2^-22), not to an
    ulp bound."""
    y = oracle_math(SOFTPLUS, xs)
    hi, lo = xs > SOFTPLUS_T, xs < -SOFTPLUS_T
    mid = ~hi & ~lo
    assert same_bits(y[hi], xs[hi]).all()
    ex = oracle_math(EXP, xs)
    assert same_bits(y[lo], ex[lo]).all()
    assert same_bits(y[mid], oracle_math(LOG, (ex[mid] + np.float32(1)).astype(np.float32))).all()
    neg = mid & (xs < 0)
    ref = np.logaddexp(0.0, xs[neg].astype(np.float64))
    assert np.max(np.abs(y[neg] - ref)) <= 2.0 ** -22
    assert np.all(y[np.isfinite(xs)] >= 0)


def test_exp_subnormal_outputs_and_log_subnormal_inputs(xs):
    """The gradual-underflow branch of mog_expf (results below FLT_MIN, down
    to x = -103.97) and mog_logf's rescaling of subnormal inputs stay within
    the functions' bounds; exp is exactly 0 below its low threshold."""
    x = xs[(xs < -87.4) & (xs >= np.float32(-103.972084045410156))]
    got = oracle_math(EXP, x)
    ref = np.exp(x.astype(np.float64))
    sub = ref.astype(np.float32) < FLT_MIN
    assert sub.sum() > 10000
    assert np.max(_ulp_err(got[sub], ref[sub])) <= BOUND[EXP]
    assert np.all(oracle_math(EXP, xs[xs < np.float32(-103.972084045410156)]) == 0)
    s = xs[(xs > 0) & (xs < FLT_MIN)]
    assert s.size >= 64
    assert np.max(_ulp_err(oracle_math(LOG, s), np.log(s.astype(np.float64)))) <= BOUND[LOG]


def test_expm1_branches(xs):
    y = oracle_math(EXPM1, xs)
    assert np.all(y[xs < -17] == -1)
    far = (np.abs(xs) >= np.float32(0.3465735912322998)) & (xs >= -17)
    assert same_bits(y[far], oracle_math(EXP, xs[far]) - np.float32(1)).all()
    tiny = (np.abs(xs) < 2.0 ** -60) & (xs != 0)
    assert same_bits(y[tiny], xs[tiny]).all()
