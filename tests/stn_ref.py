"""TEST INFRASTRUCTURE ONLY -- the spatial transformer (air/transformer.py:18-175)
restated in numpy for the kernel tests of csrc/stn.hip.

The forward is defined op for op in fp32 (oracle/air_ref.c oracle_stn,
csrc/stn_geom.h stn_tap): the grid, the source coordinates, their floors and
the clipped corners are fp32 results.  A gradient reference that recomputes
them in float64 moves every coordinate by up to an ulp of its magnitude, which
is large against a small interpolation weight, so it cannot bound a kernel's
summation error.  The reference here shares the forward's fp32 geometry
(``stn_geometry``: numpy float32, one rounding per operation, in the oracle's
order) and differs from the kernels only in how it sums: ``stn_backward64``
adds in float64 and returns, with every output, the sum of the absolute values
of its addends (the magnitude an error bound is relative to) and the count of
its non-zero addends."""
import numpy as np

F = np.float32
_CLAMP = F(1073741824.0)


def linspace32(n: int) -> np.ndarray:
    """TF LinSpace(-1, 1, n) in fp32 (linspace_at / mog_linspace): -1 for
    n == 1, else -1 + step * i with the last element set to 1."""
    if n == 1:
        return np.array([-1.0], F)
    step = F(2.0) / F(n - 1)
    v = F(-1.0) + step * np.arange(n, dtype=F)
    v[-1] = F(1.0)
    return v.astype(F)


def stn_geometry(theta, Hin, Win, Hout, Wout):
    """fp32 sampling geometry of N images: xt [Wout], yt [Hout], the source
    coordinates x, y [N, Hout, Wout] (fp32), the clipped integer corners
    x0, x1, y0, y1 and the half extents wm2 = (Win - 1.001f) / 2, hm2."""
    th = np.ascontiguousarray(theta, F).reshape(-1, 6)
    xt, yt = linspace32(Wout), linspace32(Hout)
    X, Y = xt[None, None, :], yt[None, :, None]
    c = [th[:, k][:, None, None] for k in range(6)]
    xs = (c[0] * X + c[1] * Y) + c[2] * F(1.0)
    ys = (c[3] * X + c[4] * Y) + c[5] * F(1.0)
    wm, hm = F(Win) - F(1.001), F(Hin) - F(1.001)
    x = ((xs + F(1.0)) * wm) / F(2.0)
    y = ((ys + F(1.0)) * hm) / F(2.0)
    assert x.dtype == F and y.dtype == F
    fx = np.clip(np.floor(x), -_CLAMP, _CLAMP).astype(np.int64)
    fy = np.clip(np.floor(y), -_CLAMP, _CLAMP).astype(np.int64)
    x0, x1 = np.clip(fx, 0, Win - 1), np.clip(fx + 1, 0, Win - 1)
    y0, y1 = np.clip(fy, 0, Hin - 1), np.clip(fy + 1, 0, Hin - 1)
    return dict(xt=xt, yt=yt, x=x, y=y, x0=x0, x1=x1, y0=y0, y1=y1, wm2=wm / F(2.0),
                hm2=hm / F(2.0))


def _weights32(g):
    """ax = x1f - x, bx = x - x0f, ay, by: one fp32 subtraction each."""
    x, y = g["x"], g["y"]
    return (g["x1"].astype(F) - x, x - g["x0"].astype(F), g["y1"].astype(F) - y,
            y - g["y0"].astype(F))


def _corners(U, g, Win):
    n = np.arange(U.shape[0])[:, None, None]
    flat = U.reshape(U.shape[0], -1)
    idx = (g["y0"] * Win + g["x0"], g["y1"] * Win + g["x0"], g["y0"] * Win + g["x1"],
           g["y1"] * Win + g["x1"])
    return idx, tuple(flat[n, i] for i in idx)


def stn_forward32(U, theta, out_hw):
    """transformer() in fp32, bit for bit the C oracle's: U [N, Hin, Win],
    theta [N, 6] -> [N, Hout, Wout]."""
    U = np.ascontiguousarray(U, F)
    N, Hin, Win = U.shape
    g = stn_geometry(theta, Hin, Win, *out_hw)
    ax, bx, ay, by = _weights32(g)
    _, (Ia, Ib, Ic, Id) = _corners(U, g, Win)
    wa, wb, wc, wd = ax * ay, ax * by, bx * ay, bx * by
    out = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id
    assert out.dtype == F
    return out


def stn_backward64(U, theta, G, gscale, out_hw):
    """Gradient of sum(G * gscale * transformer(U, theta)) over the fp32
    geometry, summed in float64, and dot = sum(G * forward32).

    Returns a dict: dU [N, Hin*Win], dtheta [N, 6], dot [N], each with
    ``*_mag`` (the same sum with every addend in absolute value at its
    innermost level) and ``*_cnt`` (its number of non-zero addends)."""
    U = np.ascontiguousarray(U, F)
    N, Hin, Win = U.shape
    Hout, Wout = out_hw
    G = np.ascontiguousarray(G, F).reshape(N, Hout, Wout)
    sc = np.ones(N, F) if gscale is None else np.ascontiguousarray(gscale, F)
    geo = stn_geometry(theta, Hin, Win, Hout, Wout)
    D = np.float64
    ax, bx, ay, by = (w.astype(D) for w in _weights32(geo))
    idx, (Ia, Ib, Ic, Id) = _corners(U, geo, Win)
    Ia, Ib, Ic, Id = (v.astype(D) for v in (Ia, Ib, Ic, Id))
    degen = (geo["x0"] == geo["x1"]) | (geo["y0"] == geo["y1"])
    g32 = G * sc[:, None, None]
    assert g32.dtype == F
    g = np.where(degen, 0.0, g32.astype(D))

    dU = np.zeros((N, Hin * Win), D)
    dU_mag = np.zeros_like(dU)
    dU_cnt = np.zeros((N, Hin * Win), np.int64)
    n = np.broadcast_to(np.arange(N)[:, None, None], g.shape)
    for i, w in zip(idx, (ax * ay, ax * by, bx * ay, bx * by)):
        c = w * g
        np.add.at(dU, (n, i), c)
        np.add.at(dU_mag, (n, i), np.abs(c))
        np.add.at(dU_cnt, (n, i), (c != 0).astype(np.int64))

    wm2, hm2 = D(geo["wm2"]), D(geo["hm2"])
    tx1, tx2 = ay * (Ic - Ia), by * (Id - Ib)
    ty1, ty2 = ax * (Ib - Ia), bx * (Id - Ic)
    dx = g * (tx1 + tx2) * wm2
    dy = g * (ty1 + ty2) * hm2
    mx = np.abs(g) * (np.abs(tx1) + np.abs(tx2)) * wm2
    my = np.abs(g) * (np.abs(ty1) + np.abs(ty2)) * hm2
    xt = geo["xt"].astype(D)[None, None, :]
    yt = geo["yt"].astype(D)[None, :, None]
    one = np.ones((1, 1, 1), D)
    dth = np.zeros((N, 6), D)
    dth_mag = np.zeros((N, 6), D)
    dth_cnt = np.zeros((N, 6), np.int64)
    for k, (d, m, t) in enumerate(((dx, mx, xt), (dx, mx, yt), (dx, mx, one),
                                   (dy, my, xt), (dy, my, yt), (dy, my, one))):
        dth[:, k] = (d * t).sum((1, 2))
        dth_mag[:, k] = (m * np.abs(t)).sum((1, 2))
        dth_cnt[:, k] = ((d * t) != 0).sum((1, 2))

    v = stn_forward32(U, theta, out_hw).astype(D)
    p = G.astype(D) * v
    return dict(dU=dU, dU_mag=dU_mag, dU_cnt=dU_cnt, dtheta=dth, dtheta_mag=dth_mag,
                dtheta_cnt=dth_cnt, dot=p.sum((1, 2)), dot_mag=np.abs(p).sum((1, 2)),
                dot_cnt=(p != 0).sum((1, 2)), forward=v.astype(F), geometry=geo)
