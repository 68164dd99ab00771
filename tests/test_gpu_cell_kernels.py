"""The small per-step kernels (csrc/air_cell.hip, csrc/optim.hip) on their own,
through torch.ops.mog_air.*, at the shapes and values the model runs never
give them: the scalar paths of recon_loss and batch_mean, the grid-stride
loops of the batched fill / copy / transpose, clip-Adam's ragged tails and
chunk boundaries, saturated LSTM gates, extreme VAE log-variances.

"Restatement" below means numpy float32, one rounding per operation in the
kernel's order, transcendentals through the oracle's oracle_math_vec (the
gcc compilation of include/mog_math.h)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_torch as at

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from math_spec_cases import EXP, SIGMOID, TANH, oracle_math  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _ops():
    import mog_air.torch_ops  # noqa: F401


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: "
                             f"{got[i]!r} vs {want[i]!r}")


# ---------------------------------------------------------------- LSTM ----
LSTM_SHAPES = [(1, 1), (3, 5), (1, 255), (1, 257), (7, 64), (2, 256)]
SATURATING = np.array([9.1, -9.1, 20, -20, 89, -89, 100, -100], F)


def _gates(rng, B, H):
    """N(0, 1) gates, a tenth of them saturating (every value at least once
    where the array has room)."""
    G = rng.standard_normal((B, 4 * H)).astype(F)
    m = rng.random(G.shape) < 0.1
    G[m] = rng.choice(SATURATING, int(m.sum()))
    if G.size >= 80:
        G.reshape(-1)[rng.choice(G.size, 8, replace=False)] = SATURATING
    else:
        G.reshape(-1)[rng.integers(G.size)] = rng.choice(SATURATING)
    return G


def _lstm_inputs(B, H, seed):
    rng = np.random.default_rng(seed)
    return dict(G=_gates(rng, B, H), bias=(rng.standard_normal(4 * H) * 0.5).astype(F),
                c_prev=rng.standard_normal((B, H)).astype(F),
                dh=rng.standard_normal((B, H)).astype(F), dc=rng.standard_normal((B, H)).astype(F),
                dGsum=rng.standard_normal((B, 4 * H)).astype(F),
                parts=rng.standard_normal((4, B, H)).astype(F))


def _lstm_fwd_restated(G, bias, c_prev, H):
    g = G if bias is None else G + bias[None, :]
    gi, gj, gf, go = (g[:, k * H:(k + 1) * H] for k in range(4))
    c0 = np.zeros_like(gi) if c_prev is None else c_prev
    nc = c0 * oracle_math(SIGMOID, gf + F(1)) + oracle_math(SIGMOID, gi) * oracle_math(TANH, gj)
    return nc, oracle_math(TANH, nc) * oracle_math(SIGMOID, go)


@pytest.mark.parametrize("B,H", LSTM_SHAPES)
def test_lstm_cell_forward_bit_exact(B, H):
    ops = torch.ops.mog_air
    a = _lstm_inputs(B, H, 1000 * B + H)
    assert np.isin(a["G"], SATURATING).any()
    for use_bias in (False, True):
        for use_c in (False, True):
            bias = a["bias"] if use_bias else None
            cp = a["c_prev"] if use_c else None
            c_ref, h_ref = _lstm_fwd_restated(a["G"], bias, cp, H)
            c = torch.full((B, H), float("nan"), device=DEV)
            h = torch.full((B, H), float("nan"), device=DEV)
            ops.lstm_cell_forward_(dev(a["G"]), dev(bias), dev(cp), c, h, B, H)
            assert_bits(host(c), c_ref, f"c bias={use_bias} c_prev={use_c}")
            assert_bits(host(h), h_ref, f"h bias={use_bias} c_prev={use_c}")


def _lstm_bwd64(G, bias, c_prev, dh, dc, H):
    d = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    G64 = d(G).requires_grad_()
    c64 = (d(c_prev) if c_prev is not None else torch.zeros(dh.shape, dtype=torch.float64))
    c64.requires_grad_()
    g = G64 if bias is None else G64 + d(bias)
    gi, gj, gf, go = torch.split(g, H, 1)
    c = c64 * torch.sigmoid(gf + 1.0) + torch.sigmoid(gi) * torch.tanh(gj)
    h = torch.tanh(c) * torch.sigmoid(go)
    loss = (h * d(dh)).sum()
    if dc is not None:
        loss = loss + (c * d(dc)).sum()
    loss.backward()
    return G64.grad.numpy(), c64.grad.numpy()


@pytest.mark.parametrize("B,H", LSTM_SHAPES)
def test_lstm_cell_backward_vs_float64_and_parts(B, H):
    ops = torch.ops.mog_air
    a = _lstm_inputs(B, H, 1000 * B + H)
    for use_bias, use_c, use_dc, use_sum in ((False, False, False, False), (True, True, True, True),
                                             (False, True, False, True), (True, False, True, False)):
        bias = a["bias"] if use_bias else None
        cp = a["c_prev"] if use_c else None
        dc = a["dc"] if use_dc else None
        what = f"bias={use_bias} c_prev={use_c} dc={use_dc} dGsum={use_sum}"
        c_cur, _ = _lstm_fwd_restated(a["G"], bias, cp, H)
        tG, tb, tcp, tcc, tdh, tdc = (dev(x) for x in (a["G"], bias, cp, c_cur, a["dh"], dc))

        def run(dh_t, parts=None, nparts=0):
            dG = torch.full((B, 4 * H), float("nan"), device=DEV)
            dcp = torch.full((B, H), float("nan"), device=DEV)
            gs = dev(a["dGsum"]) if use_sum else None
            if parts is None:
                ops.lstm_cell_backward_(tG, tb, tcp, tcc, dh_t, tdc, dG, dcp, gs, B, H)
            else:
                ops.lstm_cell_backward_parts_(tG, tb, tcp, tcc, dh_t, parts, nparts, tdc, dG, dcp,
                                              gs, B, H)
            return host(dG), host(dcp), None if gs is None else host(gs)

        dG, dcp, gs = run(tdh)
        dG64, dc64 = _lstm_bwd64(a["G"], bias, cp, a["dh"], dc, H)
        assert np.isfinite(dG).all() and np.isfinite(dcp).all(), what
        np.testing.assert_allclose(dG, dG64, rtol=1e-4, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(dcp, dc64, rtol=1e-4, atol=1e-6, err_msg=what)
        if use_sum:  # dGsum += dG: one fp32 add onto what it held
            assert_bits(gs, a["dGsum"] + dG, "dGsum " + what)
        # the parts form: dh + p0 + p1 .. summed in part order, then the same kernel
        for nparts in (1, 2, 3, 4):
            dh_sum = a["dh"].copy()
            for j in range(nparts):
                dh_sum = dh_sum + a["parts"][j]
            want = run(dev(dh_sum))
            got = run(tdh, dev(a["parts"][:nparts]), nparts)
            for g_, w_, n_ in zip(got, want, ("dG", "dc_prev", "dGsum")):
                if w_ is not None:
                    assert_bits(g_, w_, f"{n_} nparts={nparts} {what}")


# ---------------------------------------------------------- VAE sample ----
V_PM, V_PV = 0.1, 0.5
V_PLV = float(np.log(F(V_PV)))


def _vae_inputs(B, Z, seed):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((B, Z)).astype(F)
    eps = rng.standard_normal((B, Z)).astype(F)
    lv = (rng.standard_normal((B, Z)) * 1.5).astype(F)
    special = np.array([-104, -90, 0, 80], F)
    idx = rng.choice(B * Z, min(B * Z, 4), replace=False)
    lv.reshape(-1)[idx] = special[:idx.size] if B * Z >= 4 else special[(B + Z) % 4]
    act = (np.arange(B) % 2 == 0).astype(F) if B > 1 else np.ones(1, F)
    return mu, lv, eps, act, rng.standard_normal(B).astype(F)


@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("Z", [1, 50, 64])
def test_vae_sample_forward_bit_exact(Z, B):
    ops = torch.ops.mog_air
    mu, lv, eps, act, rl0 = _vae_inputs(B, Z, 10 * Z + B)
    pm, pv, plv = F(V_PM), F(V_PV), F(V_PLV)
    var = oracle_math(EXP, lv)
    z_ref = mu + eps * np.sqrt(var)
    d = mu - pm
    with np.errstate(over="ignore"):
        terms = (((plv - lv) - F(1)) + var / pv) + (d * d) / pv
    s = np.zeros(B, F)
    for k in range(Z):  # the kernel's k-ordered sum
        s = s + terms[:, k]
    vkl_ref = F(0.5) * s
    rl_ref = np.where(act != 0, rl0 + vkl_ref, rl0).astype(F)
    assert np.isfinite(vkl_ref).all()
    ld = 56 if Z == 50 else Z
    z = torch.full((B, Z), float("nan"), device=DEV)
    zb = torch.full((B, ld), -7.0, device=DEV, dtype=torch.bfloat16)
    vkl = torch.full((B,), float("nan"), device=DEV)
    rl = dev(rl0)
    ops.vae_sample_forward_(B, Z, V_PM, V_PV, V_PLV, dev(mu), dev(lv), dev(eps), z, zb, ld,
                            dev(act), rl, vkl)
    assert_bits(host(z), z_ref, "z")
    assert_bits(host(vkl), vkl_ref, "vkl")
    assert_bits(host(rl), rl_ref, "runloss")
    assert torch.equal(zb[:, :Z].view(torch.int16), z.to(torch.bfloat16).view(torch.int16))
    assert (zb[:, Z:] == -7.0).all()  # the pad columns keep their sentinel
    # without the bf16 copy and the running loss
    z2 = torch.full((B, Z), float("nan"), device=DEV)
    ops.vae_sample_forward_(B, Z, V_PM, V_PV, V_PLV, dev(mu), dev(lv), dev(eps), z2, None, 0,
                            dev(act), None, vkl)
    assert_bits(host(z2), z_ref, "z (no bf16, no runloss)")
    assert_bits(host(vkl), vkl_ref, "vkl (no bf16, no runloss)")


@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("Z", [1, 50, 64])
def test_vae_sample_backward_within_rounding_of_float64(Z, B):
    """dmu = dz + w (mu - pm) / pv and dlv = dz eps sqrt(var) / 2 + w (var / pv
    - 1) / 2, w = grad_scale on active rows.  The kernel allows contraction, so
    not bitwise: each output is a sum of two terms of at most eight roundings,
    |got - float64| <= 8 * 2^-24 * (|term1| + |term2|).  That count holds
    where var / pv - 1 does not cancel and var = exp(lv) is a normal number
    (a count of relative roundings says nothing about underflow: exp(-104) is
    0 by the spec), so the log-variances keep var / pv outside (1/2, 2)
    (|lv - log pv| >= ln 2) and the forward test's -104 and -90 become -85
    and -80 here; 0 and 80 stay."""
    ops = torch.ops.mog_air
    mu, lv, eps, act, _ = _vae_inputs(B, Z, 10 * Z + B)
    lv[lv == -104] = -85
    lv[lv == -90] = -80
    near = (np.abs(lv - F(V_PLV)) < 0.7) & (lv != 0)  # (lv = 0: var / pv = 2 exactly)
    lv[near] = (F(V_PLV) + np.where(lv[near] >= F(V_PLV), 1, -1) * (0.7 + np.abs(lv[near]))
                ).astype(F)
    assert (np.abs(lv.astype(np.float64) - np.log(np.float64(F(V_PV)))) >= np.log(2.0)).all()
    rng = np.random.default_rng(Z + 100 * B)
    dz = rng.standard_normal((B, Z)).astype(F)
    gs = 1.0 / 64
    dmu = torch.full((B, Z), float("nan"), device=DEV)
    dlv = torch.full((B, Z), float("nan"), device=DEV)
    ops.vae_sample_backward_(B, Z, V_PM, V_PV, gs, dev(mu), dev(lv), dev(eps), dev(dz), dev(act),
                             dmu, dlv, None, None, 0)
    d = lambda x: x.astype(np.float64)  # noqa: E731
    w = np.where(act != 0, np.float64(F(gs)), 0.0)[:, None]
    pm, pv = np.float64(F(V_PM)), np.float64(F(V_PV))
    var = np.exp(d(lv))
    m1, m2 = d(dz), w * (d(mu) - pm) / pv
    l1, l2 = d(dz) * d(eps) * 0.5 * np.sqrt(var), w * 0.5 * (-1.0 + var / pv)
    tol = 8 * 2.0 ** -24
    em, sm = np.abs(host(dmu) - (m1 + m2)), np.abs(m1) + np.abs(m2)
    el, sl = np.abs(host(dlv) - (l1 + l2)), np.abs(l1) + np.abs(l2)
    worst = [float((e[s > 0] / s[s > 0]).max() / 2.0 ** -24) for e, s in ((em, sm), (el, sl))]
    print(f"Z={Z} B={B}: dmu {worst[0]:.2f}, dlv {worst[1]:.2f} (units of 2^-24, bound 8)")
    assert (em <= tol * sm).all() and (el <= tol * sl).all(), worst
    off = act == 0  # inactive rows carry only the dz term
    assert (l2[off] == 0).all() and (m2[off] == 0).all()
    assert_bits(host(dmu)[off], dz[off], "dmu of inactive rows")


# ---------------------------------------------------------- recon loss ----
CANVAS_SPECIALS = np.array([-0.5, -0.0, 0.0, 1e-12, 0.5, 1 - 2.0 ** -24, 1.0, 1.5], F)


def _recon_restated(c, x, gs):
    """recon_pixel (csrc/air_cell.hip) but for the two logs (the hardware log
    there, compared below against float64)."""
    e = F(1e-10)
    r = np.maximum(np.minimum(c, F(1)), F(0))
    g = -(x * (F(1) / (r + e)) - (F(1) - x) * (F(1) / ((F(1) - r) + e)))
    g = np.where((c >= 0) & (c <= 1), g * F(gs), F(0)).astype(F)
    r64, x64, e64 = r.astype(np.float64), x.astype(np.float64), np.float64(e)
    bce = -(x64 * np.log(r64 + e64) + (1 - x64) * np.log((1 - r64) + e64)).sum(1)
    mse = ((x64 - r64) ** 2).sum(1)
    return r + F(0), g, bce, mse  # (+ 0: fmaxf(-0, +0) may return either zero)


@pytest.mark.parametrize("C", [3, 7, 4, 50])  # C^2 = 9, 49: the scalar kernel; 16, 2500: 16-byte
def test_recon_loss(C):
    ops = torch.ops.mog_air
    C2 = C * C
    gs = 1.0 / 3
    for B in (1, 3):
        for nparts, rows in ((0, False), (3, False), (3, True)):
            rng = np.random.default_rng(C2 + 10 * B + nparts + rows)
            x = rng.choice(np.array([0, 1, 0.3], F), (B, C2))
            canvas = rng.uniform(-0.2, 1.2, (B, C2)).astype(F)
            sp = rng.choice(C2, CANVAS_SPECIALS.size, replace=False)
            canvas[:, sp] = CANVAS_SPECIALS
            x[:, sp[:3]] = np.array([0, 1, 0.3], F)  # (each x against a clipped pixel)
            rl = rng.standard_normal(B).astype(F)
            dig = torch.zeros(B, device=DEV, dtype=torch.int32)
            recon, dcv = (torch.full((B, C2), float("nan"), device=DEV) for _ in range(2))
            bce, mse, loss = (torch.full((B,), float("nan"), device=DEV) for _ in range(3))
            what = f"C2={C2} B={B} nparts={nparts} part_rows={rows}"
            if nparts == 0:
                cv, tcan = canvas, dev(canvas)
                ops.recon_loss_(dev(x), tcan, None, 0, 0, None, C, dev(rl), dig, None, B, C2, gs,
                                recon, bce, mse, loss, None, dcv)
                assert_bits(host(tcan), canvas, "canvas untouched " + what)
            else:
                # three step contributions; at the special pixels the later ones add +0
                parts = np.zeros((3, B, C2), F)
                parts[0] = canvas
                parts[1:] = rng.uniform(-0.3, 0.3, (2, B, C2)).astype(F)
                parts[1:, :, sp] = 0
                stored, prow = parts.copy(), None
                if rows:
                    # part t of image b holds rows [lo, hi) only (even bounds at C = 50: no
                    # 4-pixel group straddles them) and counts as +0 elsewhere; what lies
                    # there in memory is never read
                    prow = np.zeros((3, B), np.int32)
                    q = 2 if C == 50 else 1
                    for t in range(3):
                        for b in range(B):
                            lo = q * int(rng.integers(0, C // q + 1))
                            hi = q * int(rng.integers(lo // q, C // q + 1))
                            prow[t, b] = lo | (hi << 16)
                            keep = np.zeros(C2, bool)
                            keep[lo * C:hi * C] = True
                            parts[t, b, ~keep] = 0
                            stored[t, b, ~keep] = 1e30
                cv = (parts[0] + parts[1]) + parts[2]
                tcan = torch.full((B, C2), float("nan"), device=DEV)
                ops.recon_loss_(dev(x), tcan, dev(stored), 3, B * C2, dev(prow), C, dev(rl), dig,
                                None, B, C2, gs, recon, bce, mse, loss, None, dcv)
                assert_bits(host(tcan), cv, "canvas_out " + what)
            r_ref, g_ref, bce64, mse64 = _recon_restated(cv, x, gs)
            assert_bits(host(recon) + F(0), r_ref, "recon " + what)
            assert_bits(host(dcv), g_ref, "dcanvas " + what)
            outside = (cv < 0) | (cv > 1)
            assert (outside.any() or rows) and (host(dcv)[outside] == 0).all()
            assert (host(dcv)[(cv == 0) | (cv == 1)] != 0).all()  # the gradient passes at equality
            print(what, "bce rel", np.abs(host(bce) - bce64).max() / np.abs(bce64).max(),
                  "mse rel", np.abs(host(mse) - mse64).max() / np.abs(mse64).max())
            np.testing.assert_allclose(host(bce), bce64, rtol=1e-5, atol=0, err_msg=what)
            np.testing.assert_allclose(host(mse), mse64, rtol=1e-5, atol=0, err_msg=what)
            assert_bits(host(loss), rl + host(bce), "loss == runloss + bce " + what)


# ---------------------------------------------------------- batch mean ----
@pytest.mark.parametrize("B", [1, 3, 4, 1023, 1024, 1028, 4100])
def test_batch_mean(B):
    """|got - float64 mean| <= (B + 1) 2^-24 mean|x|: B - 1 additions, the
    rounding of 1 / B and the product, each at most 2^-24 relative."""
    ops = torch.ops.mog_air
    rng = np.random.default_rng(B)
    x = [(rng.standard_normal(B) * s + o).astype(F) for s, o in ((1, 0), (3, 1), (0.1, -2), (10, 0))]
    for shift in (0, 1):  # 16-byte aligned, and a one-element-offset view (the scalar path)
        ts = []
        for a in x:
            buf = torch.zeros(B + 4, device=DEV)
            buf[shift:shift + B] = dev(a)
            ts.append(buf[shift:shift + B])
            assert ts[-1].data_ptr() % 16 == 4 * shift
        for present in ((1, 1, 1, 1), (1, 0, 1, 0), (0, 0, 0, 1)):
            out = torch.full((4,), -7.0, device=DEV)
            ops.batch_mean_(*[t if p else None for t, p in zip(ts, present)], B, out)
            got = host(out)
            for k in range(4):
                if not present[k]:
                    assert got[k] == -7.0  # an absent array's slot is not written
                    continue
                a64 = x[k].astype(np.float64)
                assert abs(got[k] - a64.mean()) <= (B + 1) * 2.0 ** -24 * np.abs(a64).mean(), \
                    (B, shift, present, k, got[k], a64.mean())


# ----------------------------------------------- fill / copy / transpose ----
LENGTHS = [0, 1, 3, 4, 5, 1023, 2 ** 21 + 5, 2]  # 2^21 + 5 words: past the 2048-block grid


def _framed(n, start, fill):
    """An int32 buffer with the n-word destination at word `start` (4: 16-byte
    aligned; 1: offset by one element) and sentinel words around it."""
    buf = torch.full((start + n + 3,), fill, device=DEV, dtype=torch.int32)
    return buf, buf[start:start + n]


@pytest.mark.parametrize("start", [4, 1], ids=["aligned", "offset"])
def test_fill32_batch(start):
    bufs = [_framed(n, start, -1234567) for n in LENGTHS]
    vals = [0x7FC00000 + j if j % 2 else 0xDEADBEE0 + j for j in range(len(LENGTHS))]
    torch.ops.mog_air.fill32_batch_([d for _, d in bufs], vals)
    for (buf, _), n, v in zip(bufs, LENGTHS, vals):
        want = np.full(start + n + 3, -1234567, np.int32)
        want[start:start + n] = np.array([v], np.uint32).view(np.int32)[0]
        np.testing.assert_array_equal(host(buf), want, err_msg=f"n={n}")


@pytest.mark.parametrize("dst_start,src_start", [(4, 4), (1, 4), (4, 1), (1, 1)])
def test_copy32_batch(dst_start, src_start):
    rng = np.random.default_rng(7)
    bufs = [_framed(n, dst_start, -1234567) for n in LENGTHS]
    data = [rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) for n in LENGTHS]
    srcs = []
    for n, a in zip(LENGTHS, data):
        sb, sv = _framed(n, src_start, 99)
        sv.copy_(dev(a)) if n else None
        srcs.append(sv)
    torch.ops.mog_air.copy32_batch_([d for _, d in bufs], srcs)
    for (buf, _), n, a in zip(bufs, LENGTHS, data):
        want = np.full(dst_start + n + 3, -1234567, np.int32)
        want[dst_start:dst_start + n] = a
        np.testing.assert_array_equal(host(buf), want, err_msg=f"n={n}")


def test_transpose32_batch():
    rng = np.random.default_rng(8)
    shapes = [(1, 1), (1, 7), (50, 256), (3, 0), (600, 500)]  # 300 000 > the 262 144-thread grid
    src = [dev(rng.standard_normal(s).astype(F)) for s in shapes]
    dst = [torch.full((c, r), float("nan"), device=DEV) for r, c in shapes]
    torch.ops.mog_air.transpose32_batch_(dst, src)
    for s, d in zip(src, dst):
        assert_bits(host(d), host(s).T, f"transpose {tuple(s.shape)}")


# ----------------------------------------------------------- clip-Adam ----
ADAM_LENS = [1, 2, 3, 5, 4095, 4096, 4097, 8193]
# (tensor, element): a 16-byte quad, ragged tails, either side of a chunk boundary
PLANTED = [(3, 1, np.inf), (3, 4, np.nan), (2, 2, -np.inf), (6, 4096, np.nan), (7, 10, np.nan),
           (7, 4095, np.inf), (7, 4096, -np.inf), (7, 8192, np.inf), (4, 4094, np.nan)]
ZERO_GRAD = 5  # the tensor whose gradient is all zero
B1, B2 = float(F(0.9)), float(F(0.999))  # the betas the kernel receives (fp32)


def _adam_store(seed, plant):
    from mog_air.params import ParamStore
    specs = [(f"t{i}", (n,)) for i, n in enumerate(ADAM_LENS)]
    st = ParamStore(specs, DEV)
    rng = np.random.default_rng(seed)
    state = {}
    for k, scale in (("flat", 1.0), ("grad", 3.0), ("m", 0.1)):
        state[k] = {n: (rng.standard_normal(s) * scale).astype(F) for n, s in specs}
    state["v"] = {n: rng.uniform(1e-4, 1e-2, s).astype(F) for n, s in specs}
    state["grad"][f"t{ZERO_GRAD}"][:] = 0
    if plant:
        for t, i, val in PLANTED:
            state["grad"][f"t{t}"][i] = val
    for k, d in state.items():
        hostbuf = np.zeros(st.total, F)
        for n, s in specs:
            hostbuf[st.offsets[n]:st.offsets[n] + s[0]] = d[n]
        getattr(st, k).copy_(torch.from_numpy(hostbuf))
    # step 3: the beta powers the reference step forms (fp32)
    st.beta1_power = F(0.9) ** F(3)
    st.beta2_power = F(0.999) ** F(3)
    return st, specs, state


def _adam_read(st, specs, buf):
    h = host(getattr(st, buf))
    return {n: h[st.offsets[n]:st.offsets[n] + s[0]].copy() for n, s in specs}


def test_clip_adam_table_of_tensors():
    lr, clip = 1e-3, 1.0
    st, specs, state = _adam_store(3, plant=True)
    st.apply_adam(lr, clip)
    d = lambda k: {n: torch.tensor(a, dtype=torch.float64) for n, a in state[k].items()}  # noqa: E731
    P, G, M, V = d("flat"), d("grad"), d("m"), d("v")
    at.tf_clip_adam_step(P, G, M, V, 3, lr=lr, clip=clip, beta1=B1, beta2=B2)
    got = {k: _adam_read(st, specs, k) for k in ("flat", "grad", "m", "v")}
    for n, _ in specs:
        for k, ref in (("flat", P), ("m", M), ("v", V)):
            assert np.isfinite(got[k][n]).all(), (k, n)
            np.testing.assert_allclose(got[k][n], ref[n].numpy(), rtol=1e-6, atol=1e-7,
                                       err_msg=f"{k} {n}")
    for t, i, _ in PLANTED:  # Inf / NaN gradients are zeroed in place, the rest kept
        assert got["grad"][f"t{t}"][i] == 0
    for n, _ in specs:
        keep = np.isfinite(state["grad"][n])
        assert_bits(got["grad"][n][keep], state["grad"][n][keep], "grads kept " + n)
    # padding between the tensors is not touched
    used = np.zeros(st.total, bool)
    for n, s in specs:
        used[st.offsets[n]:st.offsets[n] + s[0]] = True
    for k in ("flat", "grad", "m", "v"):
        assert (host(getattr(st, k))[~used] == 0).all(), k
    # a second identical run: the same bits
    st2, _, _ = _adam_store(3, plant=True)
    st2.apply_adam(lr, clip)
    for k in ("flat", "grad", "m", "v"):
        assert torch.equal(getattr(st, k).view(torch.int32), getattr(st2, k).view(torch.int32)), k


def test_adam_without_clip_table_of_tensors():
    """gradient_clipping_norm=None (a null sumsq): plain ApplyAdam, no
    sanitising, on finite gradients."""
    lr = 1e-3
    st, specs, state = _adam_store(4, plant=False)
    st.apply_adam(lr, None)
    b1p, b2p = np.float64(F(B1) ** F(3)), np.float64(F(B2) ** F(3))
    lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    for n, _ in specs:
        p, g, m, v = (state[k][n].astype(np.float64) for k in ("flat", "grad", "m", "v"))
        m = m + (g - m) * (1.0 - B1)
        v = v + (g * g - v) * (1.0 - B2)
        p = p - (m * lr_t) / (np.sqrt(v) + 1e-8)
        got = {k: _adam_read(st, specs, k)[n] for k in ("flat", "grad", "m", "v")}
        for k, ref in (("flat", p), ("m", m), ("v", v)):
            np.testing.assert_allclose(got[k], ref, rtol=1e-6, atol=1e-7, err_msg=f"{k} {n}")
        assert_bits(got["grad"], state["grad"][n], "grads untouched " + n)
