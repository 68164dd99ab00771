"""Device bits == host bits for the project's numerics headers.

Every bit-exact test of this suite assumes that include/mog_math.h and
csrc/step_math.h give the same bits compiled by gcc for the oracle and by
hipcc for gfx950.  Here that is checked directly, through the test-only probe
kernel mog_math_probe (csrc/testlib/instruments.hip), at the edges the model
runs never reach: overflow and gradual underflow of exp, subnormal arguments
of log, every branch constant +-2 ulps, u = 0 and 1 of the logistic noise, the
non-finite guard of lse0.  All comparisons are bitwise (both-NaN counts as
equal); there are no tolerances.

The probe is built with the product's compiler flags (no SLP-vectorised
variant, though vae_step.o is built with SLP vectorisation)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from math_spec_cases import EXP, LOG, NAMES, oracle_math, same_bits, spec_inputs  # noqa: E402
from math_spec_cases import logistic_noise as _logistic_noise  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _probe(fn, *arrays, **kw):
    from mog_air import ops
    ts = [torch.tensor(np.ascontiguousarray(a, F), device=DEV) for a in arrays]
    return ops.math_probe(fn, *ts, **kw).cpu().numpy()


def _assert_same(got, want, inputs, what):
    bad = ~same_bits(got, want)
    if bad.any():
        i = np.flatnonzero(bad)[:8]
        rows = [(tuple(repr(F(a[j])) for a in inputs), hex(int(got.view(np.uint32)[j])),
                 hex(int(want.view(np.uint32)[j]))) for j in i]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; "
                             f"(inputs, device, host): {rows}")


@pytest.fixture(scope="module")
def xs():
    return spec_inputs()


@pytest.mark.parametrize("fn", range(7), ids=NAMES)
def test_mog_math_device_equals_host(fn, xs):
    assert xs.size > 430000
    _assert_same(_probe(fn, xs), oracle_math(fn, xs), (xs,), NAMES[fn])


def test_concrete_kl_device_equals_host():
    mags = [0.0, 1e-3, 1.0, 20.0, 100.0]
    ys = [s * m for m in mags for s in (1.0, -1.0)]
    los = [-100.0, -10.0, -0.01, 0.0, 10.0, 100.0]
    temps = [0.1, 1.0, 10.0]
    grid = np.array(list(itertools.product(ys, los, temps, los, temps)), F)
    cols = [np.ascontiguousarray(grid[:, j]) for j in range(5)]
    assert np.signbit(cols[0]).sum() == grid.shape[0] // 2  # -0 is there
    want = np.array([ao._load().oracle_concrete_kl(*(float(v) for v in row)) for row in grid], F)
    assert np.isfinite(want).all()
    _assert_same(_probe("concrete_kl", *cols), want, cols, "concrete_kl")


def _lse0(a):
    with np.errstate(invalid="ignore"):
        m = np.where(a > 0, a, F(0)).astype(F)
        m = np.where((m - m) == 0, m, F(0)).astype(F)
        s = oracle_math(EXP, F(0) - m) + oracle_math(EXP, a - m)
        return oracle_math(LOG, s) + m


def test_logistic_noise_device_equals_restatement():
    u = np.array([0.0, 2.0 ** -149, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0], F)
    want = _logistic_noise(u)
    assert np.isfinite(want).all() and want[0] == -want[-1] and want[3] == 0
    _assert_same(_probe("logistic_noise", u), want, (u,), "logistic_noise")


def test_lse0_device_equals_restatement():
    a = np.array([np.inf, -np.inf, 100.0, -100.0, 0.0, -0.0, 88.0, -104.0, 1e-3], F)
    want = _lse0(a)
    assert want[0] == np.inf and want[1] == 0 and want[2] == 100 and want[3] == 0
    _assert_same(_probe("lse0", a), want, (a,), "lse0")


def test_gauss_kl_term_device_equals_restatement():
    lvs = [-104.0, -88.0, 0.0, 88.0]
    grid = np.array(list(itertools.product([float(np.log(F(0.05))), 0.0], lvs, [0.05, 1.0],
                                           [-3.0, 0.0, 0.3], [0.0, 1.5])), F)
    plv, lv, pv, mean, pm = (np.ascontiguousarray(grid[:, j]) for j in range(5))
    var = oracle_math(EXP, lv)
    assert (var[lv == -104] == 0).all() and (var[lv == -88] < 1.2e-38).all()  # 0, subnormal
    d = mean - pm
    with np.errstate(over="ignore"):  # exp(88) / 0.05 overflows to +inf, on the device as here
        want = (((plv - lv) - F(1)) + var / pv) + (d * d) / pv
    assert want.dtype == F and not np.isnan(want).any() and np.isinf(want).any()
    _assert_same(_probe("gauss_kl_term", plv, lv, var, pv, mean, pm), want,
                 (plv, lv, var, pv, mean, pm), "gauss_kl_term")


@pytest.mark.parametrize("ldw", [1, 7])
@pytest.mark.parametrize("K", [0, 1, 31, 32, 33, 64, 65, 100])
def test_chain_dot_device_equals_oracle_dense(K, ldw):
    rng = np.random.default_rng(100 * K + ldw)
    n = 300  # two blocks, the second ragged
    a = (rng.standard_normal((n, K)) * 10.0 ** rng.integers(-3, 4, (n, K))).astype(F)
    w = rng.standard_normal(max(K, 1) * ldw).astype(F)
    want = ao.dense_chain(a, w[::ldw][:K].reshape(K, 1)).ravel()
    _assert_same(_probe("chain_dot", a, w, K=K, ldw=ldw), want, (), f"chain_dot K={K}")
    if K == 64:
        _assert_same(_probe("chain64", a, w, ldw=ldw), want, (), "chain64")


def test_probe_refuses_wrong_arity():
    from mog_air import ops
    x = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        ops.math_probe("concrete_kl", x, x)
    with pytest.raises(ValueError):
        ops.math_probe("chain_dot", torch.zeros(4, 8, device=DEV), torch.zeros(8, device=DEV),
                       K=8, ldw=2)
