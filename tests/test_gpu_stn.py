"""The STN kernels (csrc/stn.hip) on every path of their run-time dispatch,
through torch.ops.mog_air.* / mog_air.ops and, for one case, the C ABI.

The shapes and theta kinds are the table of tests/stn_cases.py (read there
which path each is for; tests/test_stn_ref.py proves on the CPU that each case
reaches it).  Forward values are compared bit for bit with the C oracle.  The
backward is compared with tests/stn_ref.py stn_backward64: float64 sums over
the forward's own fp32 geometry, so reference and kernel differ only in how
they round and sum, and the bound is a count of roundings:

    |got - ref| <= (K + 1) * 2^-24 * magnitude          elementwise,

magnitude = the sum of the absolute values of the output's addends (returned
by the reference), K = the roundings between one addend and the stored sum,
the + 1 covering the second-order terms of (1 + 2^-24)^K - 1 (K < 4096).

K, counted from bwd_pixels / bwd_rows_reg / stn_bwd_image.  A lane sums
R = ceil(Hout / rp) rows per column pass (rp = 2 rows per pass for Wout <= 32,
else 1; masked rows add an exact 0) over C = ceil(Wout / (64 / rp)) passes;
mog_wave_sum adds 6 butterfly stages.

* dot: the addend G * v (v bit-identical to the forward value) is 1 rounding;
  a[6] += pv runs over R * C rows.  K_dot = R * C + 6 + 1.
* dtheta: dx = g * (ay * (Ic - Ia) + by * (Id - Ib)) * wm2 carries 5 roundings
  per inner term (subtraction, product, sum, product by g, product by wm2; g
  itself is the reference's fp32 G * gscale, wm2 the reference's fp32 value);
  the product by xt or yt is a 6th.  sdx += dx is R additions, a[0] += sdx * xt
  C more; a[1] += dx * yt is R * C.  K_dtheta = R * C + C + 6 + 6 bounds all six.
* dU: one contribution is 2 roundings ((ax * ay) * g with atomics; g * wx then
  T * wy on the separable path) and then passes through at most cnt - 1
  rounded additions in any order, cnt = the element's non-zero contributions
  (separable: (nj - 1) + (ni - 1) <= ni * nj - 1).  K_dU = cnt + 2.

Exact zeros are asserted as zeros (outputs are pre-filled with NaN): dU where
the reference has no contribution, dU and dtheta of an image whose gscale is 0
and of a window wholly outside the source.  The dot of such a window is exactly
0 only when it is outside in y (the oracle's forward is then +0 everywhere:
A - A, then C - C).  Outside in x alone its samples are degenerate, not dead:
the forward value is the oracle's cancellation residue ((A + B) - A) - B != 0
and dot, the adjoint of that forward, is its sum -- asserted within the dot
bound of the reference, and exactly 0 wherever the reference's magnitude is."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stn_cases as sc  # noqa: E402
import stn_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
U32 = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import mog_air.ops  # noqa: F401  (loads torch.ops.mog_air)


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def tbits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: "
                             f"{got[i]!r} vs {want[i]!r}")


@functools.lru_cache(maxsize=None)
def _ref(case, kind, zeros):
    """Inputs, float64 reference and oracle forward of a case: computed once,
    shared by the tests, never written to."""
    U, th, G, gs = sc.inputs(case, kind, zeros)
    ref = sr.stn_backward64(U, th, G, gs, (case.hout, case.wout))
    for a in (U, th, G, gs, *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return U, th, G, gs, ref


@functools.lru_cache(maxsize=None)
def _oracle(case, kind):
    U, th, _, _ = sc.inputs(case, kind)
    out = ao.stn(U, th, (case.hout, case.wout))
    out.setflags(write=False)
    return out


def backward(U, th, hw, G, gs, want_dU=True, u_period=0, g_period=0):
    """torch.ops.mog_air.stn_backward_ into NaN-filled outputs."""
    N, (Hin, Win) = th.shape[0], U.shape[1:]
    dU = torch.full((N, Hin * Win), NAN, device=DEV) if want_dU else None
    dth = torch.full((N, 6), NAN, device=DEV)
    dot = torch.full((N,), NAN, device=DEV)
    torch.ops.mog_air.stn_backward_(U, N, Hin, Win, th, hw[0], hw[1], G, gs, dU, dth, dot,
                                    u_period, g_period)
    return host(dU), host(dth), host(dot)


def within(got, ref, mag, K, what):
    """|got - ref| <= (K + 1) 2^-24 mag elementwise; returns the worst ratio."""
    bound = (np.asarray(K, np.float64) + 1) * U32 * mag
    err = np.abs(got.astype(np.float64) - ref)
    m = bound > 0
    ratio = float((err[m] / bound[m]).max()) if m.any() else 0.0
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} beyond the bound, worst "
                             f"{ratio:.2f} of it; first at {i}: got {got[i]!r}, reference "
                             f"{ref[i]!r}, bound {bound[i]:.3e}")
    return ratio


def check_backward(case, kind, zeros, got, what):
    """Bounds and exact zeros of (dU, dtheta, dot) against the reference."""
    dU, dth, dot = got
    _, _, _, gs, ref = _ref(case, kind, zeros)
    Kt, Kd = sc.chain_lengths(case.hout, case.wout)
    r = (within(dU, ref["dU"], ref["dU_mag"], ref["dU_cnt"] + 2, what + " dU"),
         within(dth, ref["dtheta"], ref["dtheta_mag"], Kt, what + " dtheta"),
         within(dot, ref["dot"], ref["dot_mag"], Kd, what + " dot"))
    assert (dU[ref["dU_cnt"] == 0] == 0).all(), what
    assert (dot[ref["dot_mag"] == 0] == 0).all(), what
    if kind == "outside":
        assert (dU == 0).all() and (dth == 0).all(), what
        # outside in y (images 2, 3, 4): the oracle's forward is +0 everywhere
        assert (ref["dot_mag"][2:] == 0).all() and (dot[2:] == 0).all(), what
    if zeros:
        assert (gs[::3] == 0).all()
        assert (dU[::3] == 0).all() and (dth[::3] == 0).all(), what
    return r


@pytest.mark.parametrize("case,kind", sc.CASE_KINDS, ids=sc.CASE_KIND_IDS)
def test_backward(case, kind):
    """dU, dtheta and dot within their derived bounds and exactly 0 where the
    reference has no addend, with a dense cotangent and with zeros planted in
    G and gscale; dtheta and dot without dU bit-identical to those with it."""
    hw = (case.hout, case.wout)
    for zeros in (False, True):
        U, th, G, gs, _ = _ref(case, kind, zeros)
        d = [dev(a) for a in (U, th, G, gs)]
        full = backward(d[0], d[1], hw, d[2], d[3])
        r = check_backward(case, kind, zeros, full, f"{case.name} {kind} zeros={zeros}")
        print(f"\nSTN-BOUND {case.name:13s} {kind:8s} {'zeros' if zeros else 'dense'} "
              f"dU {r[0]:.3f} dtheta {r[1]:.3f} dot {r[2]:.3f}", end="")
        _, dth, dot = backward(d[0], d[1], hw, d[2], d[3], want_dU=False)
        assert_bits(dth, full[1], "dtheta without dU")
        assert_bits(dot, full[2], "dot without dU")


def _by_name(name):
    return next(c for c in sc.CASES if c.name == name)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name,kind", [("24x40-30x64", "aligned"), ("40x28-50x64", "aligned"),
                                       ("7x9-20x24", "aligned"), ("5x5-9x11", "aligned"),
                                       ("28x28-50x50", "sheared"), ("28x28-50x50", "zoom"),
                                       ("40x40-50x50", "aligned")])
def test_backward_sigmoid_is_dU_then_sigmoid_backward(name, kind, dt):
    """dm = dU through the output sigmoid, bit for bit, on the separable path
    without the upre preload (the first two cases), with scalar staging, and
    on both atomic paths."""
    from mog_air import _lib
    from mog_air.ops import dp, stream_ptr
    case = _by_name(name)
    U, th, G, gs, _ = _ref(case, kind, True)
    N, HW, hw = U.shape[0], case.hin * case.win, (case.hout, case.wout)
    d = [dev(a) for a in (U, th, G, gs)]
    dU, dth, dot = backward(d[0], d[1], hw, d[2], d[3])
    want = torch.empty((N, HW), device=DEV, dtype=dt)
    _lib.call("mog_sigmoid_backward", dp(d[0]), dp(dev(dU)), dp(want), N * HW,
              int(dt == torch.bfloat16), stream_ptr())
    dm = torch.full((N, HW), NAN, device=DEV, dtype=dt)
    dth2 = torch.full((N, 6), NAN, device=DEV)
    dot2 = torch.full((N,), NAN, device=DEV)
    torch.ops.mog_air.stn_backward_sigmoid_(d[0], N, case.hin, case.win, d[1], hw[0], hw[1], d[2],
                                            d[3], dm, dth2, dot2, 0)
    torch.cuda.synchronize()
    assert torch.equal(tbits(dm), tbits(want))
    assert_bits(host(dth2), dth, "dtheta")
    assert_bits(host(dot2), dot, "dot")


def _mixed(rng, N):
    """aligned and sheared images in turn, so neighbouring waves take
    different paths"""
    s = rng.uniform(0.5, 0.95, (N, 2))
    t = rng.uniform(-0.5, 0.5, (N, 2))
    sh = np.where(np.arange(N) % 2 == 1, rng.uniform(0.05, 0.3, N), 0.0)
    return np.stack([s[:, 0], sh, t[:, 0], -sh, s[:, 1], t[:, 1]], 1).astype(F)


@pytest.mark.parametrize("nt", [1, 2, 3])
@pytest.mark.parametrize("which", ["u_period", "g_period"])
@pytest.mark.parametrize("shape", [(28, 28, 50, 50), (50, 50, 28, 28), (7, 9, 20, 24)])
def test_backward_periods_match_expanded_operands(shape, which, nt):
    """Image n reads row n % period of the periodic operand, and the wave
    interleave (N / period = nt > 1) changes no result: bit-identical to a
    launch without periods on the expanded operand, with and without dU."""
    Hin, Win, Hout, Wout = shape
    P = 3
    N = nt * P
    rng = np.random.default_rng(1000 + Hin + 7 * nt)
    th = dev(_mixed(rng, N))
    U = rng.uniform(0.02, 0.98, (P if which == "u_period" else N, Hin, Win)).astype(F)
    G = rng.standard_normal((P if which == "g_period" else N, Hout * Wout)).astype(F)
    gs = dev(rng.uniform(0.25, 1.5, N).astype(F)) if nt != 2 else None
    Ux = np.tile(U, (nt, 1, 1)) if which == "u_period" else U
    Gx = np.tile(G, (nt, 1)) if which == "g_period" else G
    per = {which: P}
    for want_dU in (True, False):
        got = backward(dev(U), th, (Hout, Wout), dev(G), gs, want_dU=want_dU, **per)
        want = backward(dev(Ux), th, (Hout, Wout), dev(Gx), gs, want_dU=want_dU)
        for g, w, what in zip(got, want, ("dU", "dtheta", "dot")):
            if g is not None:
                assert not np.isnan(g).any()
                assert_bits(g, w, what)


def test_backward_period_not_dividing_n_through_the_c_abi():
    """N % period != 0: rows are still read modulo the period and the
    interleave turns itself off (mog_stn_backward, called directly)."""
    from mog_air import _lib
    from mog_air.ops import dp, stream_ptr
    Hin, Win, Hout, Wout, P, N = 28, 28, 50, 50, 3, 7
    rng = np.random.default_rng(77)
    th = dev(_mixed(rng, N))
    U = dev(rng.uniform(0.02, 0.98, (N, Hin, Win)).astype(F))
    G = rng.standard_normal((P, Hout * Wout)).astype(F)
    Gx = np.concatenate([G, G, G])[:N]
    gs = dev(rng.uniform(0.25, 1.5, N).astype(F))
    dU = torch.full((N, Hin * Win), NAN, device=DEV)
    dth = torch.full((N, 6), NAN, device=DEV)
    dot = torch.full((N,), NAN, device=DEV)
    _lib.call("mog_stn_backward", dp(U), N, Hin, Win, dp(th), Hout, Wout, dp(dev(G)), dp(gs),
              dp(dU), dp(dth), dp(dot), 0, P, stream_ptr())
    torch.cuda.synchronize()
    want = backward(U, th, (Hout, Wout), dev(Gx), gs)
    for g, w, what in zip((dU, dth, dot), want, ("dU", "dtheta", "dot")):
        assert_bits(host(g), w, what)


# --------------------------------------------------------------- forward ----
def _forward(U, th, hw, out, z=None, mask=None, mode=0, n=None, u_period=0):
    N = th.shape[0] if n is None else n
    torch.ops.mog_air.stn_forward_(U, N, U.shape[1], U.shape[2], th, hw[0], hw[1], out, z, mask,
                                   mode, u_period)
    return out


@pytest.mark.parametrize("case,kind", sc.CASE_KINDS, ids=sc.CASE_KIND_IDS)
def test_forward_modes_bit_exact(case, kind):
    """mode 0 = the oracle; mode 2 = the oracle rounded to bf16; mode 1 =
    canvas + z * oracle on the active images, the others untouched."""
    U, th, _, _, _ = _ref(case, kind, False)
    want = _oracle(case, kind)
    N, hw, P = U.shape[0], (case.hout, case.wout), case.hout * case.wout
    dU_, dth = dev(U), dev(th)
    out = _forward(dU_, dth, hw, torch.full((N, P), NAN, device=DEV))
    assert_bits(host(out).reshape(want.shape), want, "mode 0")
    ob = _forward(dU_, dth, hw, torch.full((N, P), NAN, device=DEV, dtype=torch.bfloat16), mode=2)
    assert torch.equal(tbits(ob.cpu()), tbits(torch.tensor(want).to(torch.bfloat16).view(N, P)))
    rng = np.random.default_rng(5 + N + P)
    canvas = rng.standard_normal((N, P)).astype(F)
    z = rng.uniform(0.05, 1.0, N).astype(F)
    mask = (np.arange(N) % 3 != 1).astype(F)
    ref = np.where(mask[:, None] != 0, canvas + z[:, None] * want.reshape(N, P), canvas)
    cv = _forward(dU_, dth, hw, dev(canvas), dev(z), dev(mask), mode=1)
    assert_bits(host(cv), ref.astype(F), "mode 1")


@pytest.mark.parametrize("name,kind", [("28x28-50x50", "aligned"), ("7x9-20x24", "sheared"),
                                       ("28x28-40x70", "flipped"), ("50x50-28x28", "aligned")])
def test_forward_periodic_is_the_per_step_launches(name, kind):
    """n = T * N images over an N-image U (image i reads U[i % N]): the T
    per-step launches, in mode 0 and accumulating into a canvas (mode 1)."""
    case = _by_name(name)
    U, th, _, _, _ = _ref(case, kind, False)
    N, hw, P, T = U.shape[0], (case.hout, case.wout), case.hout * case.wout, 3
    tha = np.concatenate([th, th * F(0.9), th * F(1.1)]).astype(F)
    dU_ = dev(U)
    steps = [_forward(dU_, dev(tha[t * N:(t + 1) * N]), hw, torch.full((N, P), NAN, device=DEV))
             for t in range(T)]
    allr = _forward(dU_, dev(tha), hw, torch.full((T * N, P), NAN, device=DEV), n=T * N,
                    u_period=N)
    assert_bits(host(allr), np.concatenate([host(s) for s in steps]), "mode 0, u_period")
    want = np.concatenate([ao.stn(U, tha[t * N:(t + 1) * N], hw) for t in range(T)])
    assert_bits(host(allr), want.reshape(T * N, P), "mode 0 against the oracle")
    rng = np.random.default_rng(9)
    canvas = rng.standard_normal((T * N, P)).astype(F)
    z = rng.uniform(0.05, 1.0, T * N).astype(F)
    mask = (np.arange(T * N) % 4 != 2).astype(F)
    ref = np.where(mask[:, None] != 0, canvas + z[:, None] * want.reshape(T * N, P), canvas)
    cv = _forward(dU_, dev(tha), hw, dev(canvas), dev(z), dev(mask), mode=1, n=T * N, u_period=N)
    assert_bits(host(cv), ref.astype(F), "mode 1, u_period")


@pytest.mark.parametrize("case,kind", sc.CASE_KINDS, ids=sc.CASE_KIND_IDS)
def test_write_parts(case, kind):
    """stn_part_kernel on its own: the row range it records, the rows it
    stores, the rows it must not touch, and -- on the oracle -- that the rows
    it leaves out are exactly 0, so the range is sufficient."""
    U, th, _, _, _ = _ref(case, kind, False)
    want = _oracle(case, kind)
    N, Hout, Wout = U.shape[0], case.hout, case.wout
    rng = np.random.default_rng(3 + N + Hout)
    z = rng.uniform(0.05, 1.0, N).astype(F)
    mask = (np.arange(N) % 3 != 1).astype(F) if N > 1 else np.ones(1, F)
    parts = torch.full((N, Hout, Wout), NAN, device=DEV)
    rows = torch.full((N,), -12345, device=DEV, dtype=torch.int32)
    torch.ops.mog_air.stn_write_parts_(dev(U), N, case.hin, case.win, dev(th), Hout, Wout, dev(z),
                                       dev(mask), parts, rows)
    parts, rows = host(parts), host(rows)
    for n in range(N):
        if mask[n] == 0:
            assert rows[n] == 0 and np.isnan(parts[n]).all()
            continue
        lo, hi = int(rows[n]) & 0xffff, int(rows[n]) >> 16
        assert 0 <= lo <= hi <= Hout and lo % 2 == 0 and (hi % 2 == 0 or hi == Hout), (lo, hi)
        if kind == "sheared" or Hout % 2 == 1 or Hout > 64:
            assert (lo, hi) == (0, Hout)
        assert_bits(parts[n, lo:hi], z[n] * want[n, lo:hi], f"image {n} rows [{lo}, {hi})")
        assert np.isnan(parts[n, :lo]).all() and np.isnan(parts[n, hi:]).all()
        assert (want[n, :lo] == 0).all() and (want[n, hi:] == 0).all()
        if kind == "outside" and n >= 2 and Hout % 2 == 0 and Hout <= 64:
            assert lo == hi  # outside in y: nothing stored


# ------------------------------------------------------ the Hin*Win limit ----
def _big_inputs(Hin, Win, Hout, Wout, N, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.02, 0.98, (N, Hin, Win)).astype(F), _mixed(rng, N),
            rng.standard_normal((N, Hout * Wout)).astype(F), rng.uniform(0.25, 1.5, N).astype(F))


def test_backward_lds_slice_above_64k():
    """100x100 -> 16x16 with dU: one wave per workgroup and an 80,256-byte
    dynamic LDS slice; the same bounds and identities as the table."""
    case = sc.BIG
    hw = (case.hout, case.wout)
    for kind in ("aligned", "sheared"):
        U, th, G, gs, _ = _ref(case, kind, False)
        d = [dev(a) for a in (U, th, G, gs)]
        full = backward(d[0], d[1], hw, d[2], d[3])
        r = check_backward(case, kind, False, full, f"{case.name} {kind}")
        print(f"\nSTN-BOUND {case.name:13s} {kind:8s} dense dU {r[0]:.3f} dtheta {r[1]:.3f} "
              f"dot {r[2]:.3f}", end="")
        _, dth, dot = backward(d[0], d[1], hw, d[2], d[3], want_dU=False)
        assert_bits(dth, full[1], "dtheta without dU")
        assert_bits(dot, full[2], "dot without dU")


def test_backward_source_size_limit():
    """include/mog_air.h: Hin * Win <= 16384 runs (128x128, a 131,136-byte
    slice with dU); one more source row is MOG_ERR_INVALID and nothing is
    launched."""
    Hout = Wout = 4
    U, th, G, gs = _big_inputs(128, 128, Hout, Wout, 2, 5)
    ref = sr.stn_backward64(U, th, G, gs, (Hout, Wout))
    dU, dth, dot = backward(dev(U), dev(th), (Hout, Wout), dev(G), dev(gs))
    Kt, Kd = sc.chain_lengths(Hout, Wout)
    within(dU, ref["dU"], ref["dU_mag"], ref["dU_cnt"] + 2, "dU")
    within(dth, ref["dtheta"], ref["dtheta_mag"], Kt, "dtheta")
    within(dot, ref["dot"], ref["dot_mag"], Kd, "dot")
    assert (dU[ref["dU_cnt"] == 0] == 0).all()
    U, th, G, gs = _big_inputs(129, 128, Hout, Wout, 2, 6)
    for want_dU in (True, False):
        with pytest.raises(RuntimeError, match="stn_backward_"):
            backward(dev(U), dev(th), (Hout, Wout), dev(G), dev(gs), want_dU=want_dU)
    torch.cuda.synchronize()
