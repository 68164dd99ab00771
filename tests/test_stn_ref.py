"""The STN reference of the kernel tests (tests/stn_ref.py) against the two
oracles, and the case table (tests/stn_cases.py) against the geometry and the
dispatch path each case is listed for.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle import air_torch as at

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stn_cases as sc  # noqa: E402
import stn_ref as sr  # noqa: E402

F = np.float32
ALL = sc.CASE_KINDS + [(sc.BIG, k) for k in ("aligned", "sheared")]
ALL_IDS = sc.CASE_KIND_IDS + [f"{sc.BIG.name}-{k}" for k in ("aligned", "sheared")]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("case,kind", ALL, ids=ALL_IDS)
def test_forward32_is_the_c_oracle_bitwise(case, kind):
    U, th, _, _ = sc.inputs(case, kind)
    assert U.shape[0] <= 9
    ref = ao.stn(U, th, (case.hout, case.wout))
    got = sr.stn_forward32(U, th, (case.hout, case.wout))
    np.testing.assert_array_equal(_bits(got), _bits(ref))


def _autograd_over_fp32_geometry(U, th, G, gs, hw):
    """torch float64 autograd with straight-through coordinates: values,
    floors and corners are the fp32 ones, the derivative is the float64
    affine map's (x = x32 + (x64(theta) - x64(theta).detach()))."""
    N, Hin, Win = U.shape
    geo = sr.stn_geometry(th, Hin, Win, *hw)
    D = torch.float64
    T = torch.tensor(th.astype(np.float64), requires_grad=True)
    Ut = torch.tensor(U.astype(np.float64), requires_grad=True)
    xt = torch.tensor(geo["xt"].astype(np.float64)).view(1, 1, -1)
    yt = torch.tensor(geo["yt"].astype(np.float64)).view(1, -1, 1)
    c = [T[:, k].view(N, 1, 1) for k in range(6)]
    x64 = ((c[0] * xt + c[1] * yt + c[2]) + 1.0) * float(geo["wm2"])
    y64 = ((c[3] * xt + c[4] * yt + c[5]) + 1.0) * float(geo["hm2"])
    ex, ey = x64 - x64.detach(), y64 - y64.detach()
    ax32, bx32, ay32, by32 = (torch.tensor(w.astype(np.float64)) for w in sr._weights32(geo))
    ax, bx, ay, by = ax32 - ex, bx32 + ex, ay32 - ey, by32 + ey
    flat = Ut.reshape(N, -1)
    idx = lambda y, x: torch.tensor(geo[y] * Win + geo[x]).reshape(N, -1)  # noqa: E731
    Ia, Ib, Ic, Id = (torch.gather(flat, 1, idx(y, x)).view(N, *hw)
                      for y, x in (("y0", "x0"), ("y1", "x0"), ("y0", "x1"), ("y1", "x1")))
    out = ax * ay * Ia + ax * by * Ib + bx * ay * Ic + bx * by * Id
    g32 = G.reshape(N, *hw) * gs[:, None, None]
    assert g32.dtype == F
    degen = (geo["x0"] == geo["x1"]) | (geo["y0"] == geo["y1"])
    g = torch.tensor(np.where(degen, 0.0, g32.astype(np.float64)), dtype=D)
    (out * g).sum().backward()
    return Ut.grad.numpy().reshape(N, -1), T.grad.numpy()


@pytest.mark.parametrize("case,kind", ALL, ids=ALL_IDS)
def test_backward64_is_autograd_over_the_same_geometry(case, kind):
    hw = (case.hout, case.wout)
    for zeros in (False, True):
        U, th, G, gs = sc.inputs(case, kind, zeros)
        ref = sr.stn_backward64(U, th, G, gs, hw)
        dU, dth = _autograd_over_fp32_geometry(U, th, G, gs, hw)
        assert (np.abs(ref["dU"] - dU) <= 1e-12 * ref["dU_mag"]).all()
        assert (np.abs(ref["dtheta"] - dth) <= 1e-12 * ref["dtheta_mag"]).all()
        assert (ref["dU_mag"][ref["dU_cnt"] == 0] == 0).all()
        if zeros:  # gscale == 0: no gradient addend at all
            assert not ref["dU_cnt"][::3].any() and not ref["dtheta_cnt"][::3].any()


@pytest.mark.parametrize("hin,win,hout,wout", [(7, 5, 1, 6), (9, 12, 6, 1)])
def test_torch_oracle_is_the_c_oracle_at_one_row_or_column(hin, win, hout, wout):
    """linspace(-1, 1, 1) is -1 in TF, in the C oracle and in the kernels."""
    case = next(c for c in sc.CASES if (c.hin, c.win, c.hout, c.wout) == (hin, win, hout, wout))
    for kind in case.kinds:
        U, th, _, _ = sc.inputs(case, kind)
        ref = ao.stn(U, th, (hout, wout))
        got = at.transformer(torch.tensor(U), torch.tensor(th), (hout, wout)).numpy()
        np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert float(at._linspace(1, torch.float32)[0]) == -1.0
    np.testing.assert_array_equal(at._linspace(5, torch.float32).numpy(), sr.linspace32(5))


@pytest.mark.parametrize("case,kind", ALL, ids=ALL_IDS)
def test_case_geometry(case, kind):
    """Each case produces the geometry, and takes the dispatch path, that it
    is in the table for."""
    U, th, _, _ = sc.inputs(case, kind)
    N, (Hin, Win, Hout, Wout) = U.shape[0], (case.hin, case.win, case.hout, case.wout)
    assert N == sc.n_images(case, kind) and N in (1, 5, 9)
    assert len({tuple(t) for t in th}) == N
    geo = sr.stn_geometry(th, Hin, Win, Hout, Wout)
    lx, ly = geo["x0"] != geo["x1"], geo["y0"] != geo["y1"]
    live = lx & ly
    paths = [sc.dispatch(t, Hin, Win, Hout, Wout)["path"] for t in th]
    if kind in ("aligned", "zoom", "large", "tiny"):
        assert (th[:, 0] > 0).all() and (th[:, 4] > 0).all() and (th[:, 0] != th[:, 4]).all()
        assert paths == [case.path] * N
    if kind == "aligned" and min(Hin, Win) > 1:
        assert live[0].all() or min(Hout, Wout) == 1  # image 0 lies inside
        for i, side in enumerate(sc.SIDES[:N - 1], 1):
            a, b, lim = (("x0", "x1", Win - 1) if side in ("left", "right")
                         else ("y0", "y1", Hin - 1))
            edge = 0 if side in ("left", "top") else lim
            clipped = (geo[a][i] == edge) & (geo[b][i] == edge)
            other = (geo[a][i] == lim - edge) & (geo[b][i] == lim - edge)
            # a grid of one column / row sits at -1: only the left / top window reaches it
            if (Wout if side in ("left", "right") else Hout) > 1:
                assert clipped.any() and not other.any(), side
                assert (live[i].any() or min(Hout, Wout) == 1), side
    if kind == "flipped":
        assert {(bool(t[0] < 0), bool(t[4] < 0)) for t in th} >= {(True, True), (False, True)}
        want = "atomic-aligned" if Hout <= 64 else "atomic-general"
        assert paths == [want] * N
    if kind == "sheared":
        assert (th[:, 1] != 0).all() and (th[:, 3] != 0).all()
        assert np.abs(th[:, [1, 3]]).max() <= 0.3
        assert paths == ["atomic-general"] * N
    if kind == "outside":
        assert not live.any()
        assert all(p in (case.path, "atomic-aligned") for p in paths)
    if kind == "large":
        assert (~lx).any() and (~ly).any()  # the window reaches past the source
    if kind == "tiny" and min(Hin, Win) > 1:
        # 0.022 of the extent: at most one cell boundary crossed up to 46 cells, two beyond
        for a, ext in (("x0", Win), ("y0", Hin)):
            assert (np.ptp(geo[a].reshape(N, -1), axis=1) <= (1 if ext <= 46 else 2)).all()
    if case.name == "8x8-64x64" and kind == "aligned" or kind == "zoom" or \
            (case.name == "28x28-50x50" and kind == "tiny"):
        assert min(sc.columns_per_source_column(geo, n) for n in range(N)) > 8
    if case.name == "28x28-50x50" and kind == "aligned":
        assert max(sc.columns_per_source_column(geo, n) for n in range(N)) <= 8


def test_table_reaches_every_listed_path():
    """The dispatch conditions of stn_bwd_kernel, each named by a case."""
    d = {c.name: sc.dispatch(sc.thetas(c, "aligned")[0], c.hin, c.win, c.hout, c.wout)
         for c in sc.CASES + (sc.BIG,)}
    nd = {c.name: sc.dispatch(sc.thetas(c, "aligned")[0], c.hin, c.win, c.hout, c.wout, False)
          for c in sc.CASES}
    dm = {c.name: sc.dispatch(sc.thetas(c, "aligned")[0], c.hin, c.win, c.hout, c.wout, True, 1)
          for c in sc.CASES}
    assert {v["path"] for v in d.values()} == {"regs+sdu", "sdu", "atomic-aligned",
                                               "atomic-general"}
    assert nd["28x28-50x50"]["path"] == "regs+read-aligned"        # bwd_rows_reg<0>
    assert nd["50x50-28x28"]["windowed"] and not nd["7x9-20x24"]["windowed"]
    assert nd["12x20-70x33"]["path"] == "read-general"
    # regs against non-regs, windowed against whole-image staging, sdu against atomics
    fl = sc.dispatch(sc.thetas(sc.CASES[2], "flipped")[0], 24, 40, 30, 64)
    assert fl["path"] == "atomic-aligned" and nd["24x40-30x64"]["regs"]
    for name in ("24x40-30x64", "40x28-50x64"):
        assert dm[name]["sdu"] and not dm[name]["upre"]
    assert dm["28x28-50x50"]["upre"] and dm["7x9-20x24"]["upre"]
    assert not d["7x9-20x24"]["staging16"] and not d["5x5-9x11"]["staging16"]
    assert d["5x5-9x11"]["rows_per_pass"] == 2 and d["28x28-40x70"]["passes"] == 2
    assert d["72x72-20x20"]["wpb"] == 1 and d["72x72-20x20"]["slice_bytes"] <= 64 * 1024
    assert d["60x60-20x20"]["wpb"] == 2 and d["40x40-50x50"]["wpb"] == 4
    assert d["100x100-16x16"]["wpb"] == 1 and d["100x100-16x16"]["slice_bytes"] > 64 * 1024


def test_distance_to_pure_float64_autograd(capsys):
    """Why the kernels are judged against fp32 geometry:
    float64 autograd of the float64 forward is not within a summation bound
    of the fp32-geometry gradient.  Prints the distance per case; asserts
    that at 50x50 -> 28x28 sheared it is beyond anything a bound of a few
    hundred roundings (1e-5 of the magnitude) could absorb."""
    worst = {}
    for case, kind in sc.CASE_KINDS:
        if kind not in ("aligned", "sheared") or min(case.hout, case.wout) == 1:
            continue
        hw = (case.hout, case.wout)
        U, th, G, gs = sc.inputs(case, kind)
        ref = sr.stn_backward64(U, th, G, gs, hw)
        Ut = torch.tensor(U.astype(np.float64), requires_grad=True)
        out = at.transformer(Ut, torch.tensor(th.astype(np.float64)), hw)
        (out * torch.tensor((G.reshape(out.shape) * gs[:, None, None]).astype(np.float64))).sum() \
            .backward()
        m = ref["dU_mag"] > 0
        if m.any():
            worst[f"{case.name}-{kind}"] = float(
                (np.abs(Ut.grad.numpy().reshape(m.shape) - ref["dU"])[m] / ref["dU_mag"][m]).max())
    with capsys.disabled():
        print("\n|dU(float64 autograd) - dU(fp32 geometry)| / magnitude, worst element:")
        for k, v in worst.items():
            print(f"  {k:28s} {v:.2e}")
    assert worst["50x50-28x28-sheared"] > 1e-5
