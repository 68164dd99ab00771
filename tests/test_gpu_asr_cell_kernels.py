"""The AIR-ASR cell and loss kernels (csrc/asr_cell.hip) on their own, through
torch.ops.mog_air.*, at the branch points the whole-model tests never reach:
partial last blocks (B % 4 != 0, B across 256), Tx < T and Tx == 0, every hinge
of the structural terms on and off and exactly at its edge, TF's tie rules,
stopping / stopped / inactive images, live 0, the test model, fix_steps, both
scale priors, each cotangent alone.

References: tests/asr_cell_ref.py (pinned on the CPU by
tests/test_asr_cell_ref.py).  "Bit-exact" is against the numpy float32
restatements in the kernels' order.  "Within the bound" is per output column
|got - ref64| <= max(8 E32, 2^-20 max|ref64|), E32 the largest |ref32 - ref64|
of the column over the case table of one test, ref32 the same reference
function in float32 on the CPU; the tests print got's error / bound per column.

Every output buffer starts as NaN and ends in a row of sentinels past the
extent the op needs, which must stay untouched.

Measured on an MI355X, 2026-10-21 (worst error / bound over all columns):
terms random tables 0.256 (size), branch table 0.127 (dreg[lo]), step forward
0.512 (rec[skl], learned prior), step backward 0.687 (douts[sm1], dtheta_back
alone, learned prior).  No column needed more than the factor 8.  With the
columns taken per launch instead (as few as one image, E32 from that image
alone) single columns reached 3.1 (rec[zkl], B = 1) and 2.3 (douts[slv0], B =
4, dtheta_back alone): E32 over a handful of images is too noisy a measure of
float32's error, which is why a column here spans the whole case table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asr_cell_ref as R  # noqa: E402
from asr_cell_ref import Q  # noqa: E402
from test_gpu_cell_kernels import assert_bits, dev, host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAN = float("nan")
SENT = -7.25
ISENT = -77
C = 50


@pytest.fixture(scope="module", autouse=True)
def _ops():
    import mog_air.torch_ops  # noqa: F401


def nan_buf(n, extra):
    """n NaNs (the extent the op needs) and `extra` sentinels after them."""
    t = torch.full((n + extra,), NAN, device=DEV)
    t[n:] = SENT
    return t


def framed(a, extra_shape):
    """The array a with a block of sentinels after it."""
    a = np.ascontiguousarray(a)
    sent = ISENT if a.dtype.kind == "i" else SENT
    return dev(np.concatenate([a.reshape(-1), np.full(int(np.prod(extra_shape)), sent, a.dtype)]))


def sentinel_intact(t, n, what):
    tail = host(t).reshape(-1)[n:]
    assert tail.size and (tail == (ISENT if tail.dtype.kind == "i" else SENT)).all(), what


class Columns:
    """Collects (got, ref64, ref32) per column over the launches of one test."""

    def __init__(self):
        self.c = {}

    def add(self, name, got, r64, r32):
        g, a, b = (np.asarray(x, np.float64).reshape(-1) for x in (got, r64, r32))
        assert g.shape == a.shape == b.shape, (name, g.shape, a.shape, b.shape)
        self.c.setdefault(name, []).append((g, a, b))

    def check(self, what, exact_zeros=()):
        bad, worst = [], (0.0, "")
        for name, parts in self.c.items():
            g, a, b = (np.concatenate(x) for x in zip(*parts))
            assert np.isfinite(g).all(), (what, name)
            lim = R.bound(a, b)
            err = float(np.abs(g - a).max())
            ratio = err / lim if lim > 0 else (0.0 if err == 0 else np.inf)
            worst = max(worst, (ratio, name))
            print(f"{what} {name}: err {err:.3e} bound {lim:.3e} ratio {ratio:.3f}")
            if ratio > 1:
                bad.append((name, err, lim))
            if name.split("[")[0] in exact_zeros or name in exact_zeros:
                z = a == 0
                if not (g[z] == 0).all():
                    bad.append((name, "non-zero where the reference is exactly 0",
                                int((g[z] != 0).sum())))
        print(f"{what}: worst ratio {worst[0]:.3f} ({worst[1]})")
        assert not bad, (what, bad)


# ======================================================= pack / unpack ====
PACK_SHAPES = [(1, 1, 1, 5), (3, 2, 5, 12), (5, 50, 256, 320)]


@pytest.mark.parametrize("B,Z,H,ld", PACK_SHAPES)
def test_pack_bit_exact(B, Z, H, ld):
    ops = torch.ops.mog_air
    rng = np.random.default_rng(B + Z + H)
    z, ss, h, h2 = (rng.standard_normal(s).astype(F) for s in ((B, Z), (B, 3), (B, H), (B, H)))

    def want(z_, ss_, h_):
        o = np.zeros((B, ld), F)
        for src, lo in ((z_, 0), (ss_, Z), (h_, Z + 3)):
            if src is not None:
                o[:, lo:lo + src.shape[1]] = src
        return o

    for uz, us, uh in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        zz, s_, hh = (a if u else None for a, u in ((z, uz), (ss, us), (h, uh)))
        for two in (False, True):
            out, out2 = nan_buf(B * ld, ld), nan_buf(B * ld, ld)
            if two:
                ops.asr_pack_(B, Z, H, ld, dev(zz), dev(s_), dev(hh), out, dev(h2), out2)
            else:
                ops.asr_pack_(B, Z, H, ld, dev(zz), dev(s_), dev(hh), out, None, None)
            what = f"z={uz} ss={us} h={uh} two={two}"
            assert_bits(host(out)[:B * ld].reshape(B, ld), want(zz, s_, hh), "out " + what)
            sentinel_intact(out, B * ld, "out " + what)
            if two:
                assert_bits(host(out2)[:B * ld].reshape(B, ld), want(zz, s_, h2), "out2 " + what)
                sentinel_intact(out2, B * ld, "out2 " + what)
            else:
                assert torch.isnan(out2[:B * ld]).all()


@pytest.mark.parametrize("B,Z,H,ld", PACK_SHAPES)
def test_unpack_bit_exact(B, Z, H, ld):
    """dz = (dz +) (a + g), dss = a + g, dh += a, dhg += g with a, g the parts of
    dU, dUg summed in part order: four float32 additions, restated in numpy.
    The pad columns of dU / dUg hold NaN: they are not read."""
    ops = torch.ops.mog_air
    rng = np.random.default_rng(10 * B + Z)
    n = Z + 3 + H
    dU, dUg = (rng.standard_normal((4, B, ld)).astype(F) for _ in range(2))
    dU[:, :, n:], dUg[:, :, n:] = np.nan, np.nan
    dz0, dh0, dhg0 = (rng.standard_normal(s).astype(F) for s in ((B, Z), (B, H), (B, H)))
    for acc in (0, 1):
        for nparts in (1, 2, 3, 4):
            a, g = dU[0].copy(), dUg[0].copy()
            for j in range(1, nparts):
                a, g = a + dU[j], g + dUg[j]
            s = a + g
            want = {"dz": dz0 + s[:, :Z] if acc else s[:, :Z], "dss": s[:, Z:Z + 3],
                    "dh": dh0 + a[:, Z + 3:n], "dhg": dhg0 + g[:, Z + 3:n]}
            for entry in (("parts", "plain") if nparts == 1 else ("parts",)):
                dz = framed(dz0, (Z,)) if acc else nan_buf(B * Z, Z)
                dss = nan_buf(B * 3, 3)
                dh, dhg = framed(dh0, (H,)), framed(dhg0, (H,))
                tU, tUg = dev(dU[:nparts]), dev(dUg[:nparts])
                if entry == "plain":
                    ops.asr_unpack_(B, Z, H, ld, tU, tUg, dz, dss, dh, dhg, acc)
                else:
                    ops.asr_unpack_parts_(B, Z, H, ld, tU, tUg, nparts, dz, dss, dh, dhg, acc)
                what = f"acc_dz={acc} nparts={nparts} {entry}"
                for k, t in (("dz", dz), ("dss", dss), ("dh", dh), ("dhg", dhg)):
                    w = want[k]
                    assert_bits(host(t)[:w.size].reshape(w.shape), w, f"{k} {what}")
                    sentinel_intact(t, w.size, f"{k} {what}")


# ================================================================ terms ====
def _run_terms(tb, cfg, gs, inv):
    ops = torch.ops.mog_air
    B, T = tb["B"], tb["T"]
    cons, g = list(cfg.constrains_num), R.gammas(cfg)
    rec, vkl, zmask, live = dev(tb["rec"]), dev(tb["vkl"]), dev(tb["zmask"]), dev(tb["live"])
    o = {k: nan_buf(B, 1) for k in ("klsum", "pr", "area", "out", "size", "overlap", "element")}
    o["zsum"], o["margin"] = nan_buf(T, 1), nan_buf(1, 1)
    ops.asr_terms_(B, T, C, cons, g, rec, vkl, zmask, live, o["klsum"], o["pr"], o["area"],
                   o["out"], o["size"], o["overlap"], o["zsum"])
    o["loss"] = o["klsum"].clone()  # (elbo without the reconstruction term)
    ops.asr_finalize_(B, T, C, cons, g, inv, rec, live, o["zsum"], o["pr"], o["loss"],
                      o["element"], o["margin"])
    o["dreg"] = nan_buf(T * 4 * B, 4 * B)
    ops.asr_terms_backward_(B, T, C, cons, g, gs, inv, rec, live, o["zsum"], o["dreg"])
    n = {"zsum": T, "margin": 1, "dreg": T * 4 * B}
    res = {}
    for k, t in o.items():
        sentinel_intact(t, n.get(k, B), k)
        res[k] = host(t)[:n.get(k, B)]
    res["dreg"] = res["dreg"].reshape(T, 4, B)
    return res


def _check_terms(tb, cfg, gs, inv, cols, what):
    got = _run_terms(tb, cfg, gs, inv)
    args = (tb["rec"], tb["vkl"], tb["zmask"], tb["live"], cfg)
    r64 = R.terms_ref(*args, grad_scale=gs, inv_batch_global=inv)
    r32 = R.terms_ref(*args, grad_scale=gs, inv_batch_global=inv, dtype=torch.float32)
    f32 = R.terms_fwd_f32(tb["rec"], tb["live"], cfg)
    Tx = r64["Tx"]
    assert Tx == tb["Tx"]
    for k in ("area", "out", "size", "overlap", "element"):
        assert_bits(got[k], f32[k], f"{k} {what}")
    for k in ("area", "out", "size", "overlap", "element", "klsum", "pr", "loss"):
        cols.add(k, got[k], r64[k], r32[k])
    cols.add("margin", got["margin"], [r64["margin"]], [r32["margin"]])
    zp = np.abs(tb["rec"][:Tx, Q["zprob"]].astype(np.float64)).sum(1)
    assert (np.abs(got["zsum"][:Tx] - r64["zsum"]) <= tb["B"] * 2.0 ** -24 * zp).all(), what
    assert_bits(got["dreg"][Tx:], np.zeros_like(got["dreg"][Tx:]), f"dreg rows >= Tx {what}")
    for c, name in enumerate(("s", "tx", "ty", "lo")):
        cols.add(f"dreg[{name}]", got["dreg"][:Tx, c], r64["dreg"][:Tx, c], r32["dreg"][:Tx, c])
    return got, r64


TERMS_TX = {1: (0, 1), 3: (0, 1, 2, 3), 8: (0, 1, 7, 8)}


@pytest.mark.parametrize("B", [1, 255, 257])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_terms_random_table(T, B):
    """Random records across the 256-image block and the zprob sum's stride,
    Tx through live as 0, 1, T - 1 and T; records, vkl and zmask of the steps
    >= Tx are NaN (asr_zprob_sum_kernel does sum them into zsum[t >= Tx], which
    nothing reads: only zsum[:Tx] is checked).  The margin's batch mean is over
    2 B images at T = 3 (another rank's share), B otherwise.
    Worst ratio against the bound: 0.256 (size, T = 8), MI355X, 2026-10-21."""
    cols = Columns()
    cfg = R.loss_cfg(cons=(1, 3) if T < 8 else (1, 3, 8))
    inv = R.f32r(1.0 / (2 * B if T == 3 else B))
    for Tx in TERMS_TX[T]:
        tb = R.terms_random(B, T, Tx, seed=1000 * T + 10 * B + Tx)
        got, _ = _check_terms(tb, cfg, 1.0 / 64, inv, cols, f"T={T} B={B} Tx={Tx}")
        if Tx == 0:
            for k in ("klsum", "pr", "area", "out", "size", "overlap", "element", "margin"):
                assert (got[k] == 0).all(), k
    cols.check(f"terms T={T} B={B}", exact_zeros=("dreg",))


BRANCH_CFGS = [dict(cons=c) for c in R.BRANCH_CONS] + [dict(g_margin=0.0), dict(g_num=0.0)]


@pytest.mark.parametrize("ci", range(len(BRANCH_CFGS)))
def test_terms_branch_table(ci):
    """One image per branch (asr_cell_ref._geometry_rows x LO_ROWS), every
    value exact in float32, under each allowed-count set, g_margin = 0 and g_num =
    0.  dreg element by element: an exact zero of the reference (an inactive
    hinge, the losing side of a Maximum tie, the cancelled halves of a ReduceMin
    tie, a coincident centre) must be an exact zero here.
    Worst ratio against the bound: 0.127 (dreg[lo]), MI355X, 2026-10-21."""
    cols = Columns()
    cfg = R.loss_cfg(area_minmax=R.BRANCH_AREA, **BRANCH_CFGS[ci])
    tb = R.terms_branch_table()
    got, r64 = _check_terms(tb, cfg, 1.0 / 64, R.f32r(1.0 / tb["B"]), cols, f"branch cfg {ci}")
    assert (r64["dreg"] == 0).any() and (r64["dreg"] != 0).any()
    if cfg.constrains_margin_gamma == 0:
        assert (got["element"] == 0).all() and got["margin"][0] == 0
    cols.check(f"branch table cfg {ci}", exact_zeros=("dreg",))


# ================================================================= step ====
STEP_CFGS = [
    R.StepCfg(step=0, fix_steps=-1, train=True, temperature=0.1, g_num=0.5, live=1),
    R.StepCfg(step=2, fix_steps=-1, train=True, temperature=1.0, g_num=0.0, live=0),
    R.StepCfg(step=0, fix_steps=0, train=False, temperature=0.1, g_num=0.5, live=1),
    R.StepCfg(step=2, fix_steps=2, train=True, temperature=1.0, g_num=0.5, live=1),
    R.StepCfg(step=2, fix_steps=3, train=False, temperature=0.1, g_num=0.0, live=0),
    R.StepCfg(step=0, fix_steps=2, train=True, temperature=0.1, g_num=0.5, live=1),
]
STEP_B = [1, 4, 5, 7]


def _offsets(B):
    return (0, 5, 8) if B == 1 else tuple(range(0, len(R.STEP_ROWS), B))


def _rows(a, B):
    """[B, 64] rows and one row of sentinels."""
    return framed(np.asarray(a, F), (R.HS,))


def _run_step_forward(inp, cfg, learned):
    ops = torch.ops.mog_air
    B = len(inp["stop_old"])
    hid_in = [None if a is None else np.maximum(np.asarray(a, F), F(0)) for a in inp["pre"]]
    hid_in += [np.asarray(a, F) for a in inp["raw"]]
    t = {"hid": [None if a is None else _rows(a, B) for a in hid_in],
         "w": [dev(a) for a in inp["w"]], "gw": [dev(a) for a in inp["gw"]] if learned else [],
         "eps_shift": dev(inp["eps_shift"]), "eps_scale": dev(inp["eps_scale"]), "u": dev(inp["u"]),
         "stop": framed(inp["stop_old"], (1,)), "digits": framed(inp["digits"], (1,))}
    live = np.zeros(cfg.step + 2, np.int32)
    live[cfg.step] = cfg.live
    t["live"] = framed(live, (1,))
    sizes = {"rec": R.NQ * B, "theta_fwd": 6 * B, "theta_back": 6 * B, "ss": 3 * B, "scale": B,
             "shift": 2 * B, "zprob": B, "zmask": B, "zval": B, "zc": B}
    for k, n in sizes.items():
        t[k] = nan_buf(n, n // B)
    ops.asr_step_forward_(B, cfg.step, cfg.train, cfg.fix_steps, cfg.thr, cfg.temperature, cfg.gcm,
                          cfg.gcvar, cfg.gclv32, cfg.g_num, t["w"], t["gw"], t["hid"],
                          t["eps_shift"], t["eps_scale"], t["u"], t["stop"], t["digits"], t["live"],
                          *[t[k] for k in sizes])
    return t, hid_in, sizes


def _check_step_forward(inp, cfg, learned, cols, what):
    B = len(inp["stop_old"])
    t, hid_in, sizes = _run_step_forward(inp, cfg, learned)
    f32 = R.step_fwd_f32(inp, cfg, learned)
    f64, _ = R.step_ref(inp, cfg, learned)
    r32, _ = R.step_ref(inp, cfg, learned, dtype=torch.float32)
    nq = f32["rec"].shape[0]
    for k, n in sizes.items():
        sentinel_intact(t[k], n, f"{k} {what}")
    rec = host(t["rec"])[:R.NQ * B].reshape(R.NQ, B)
    assert_bits(rec[:nq], f32["rec"], "rec " + what)
    assert np.isnan(rec[nq:]).all()  # (slots 28 / 29 belong to the learned prior)
    for k in ("theta_fwd", "theta_back", "ss", "scale", "shift", "zprob", "zmask", "zval", "zc"):
        got = host(t[k])[:sizes[k]].reshape(f32[k].shape)
        assert_bits(got, f32[k], f"{k} {what}")
        cols.add(k, got, f64[k], r32[k])
    for name, i in Q.items():
        if i < nq:
            cols.add(f"rec[{name}]", rec[i], f64["rec"][i], r32["rec"][i])
    assert_bits(host(t["stop"])[:B], f32["stop"], "stop " + what)
    np.testing.assert_array_equal(host(t["digits"])[:B], f32["digits"], err_msg=what)
    np.testing.assert_array_equal(f32["digits"], f64["digits"])
    live = host(t["live"])
    want_live = np.zeros(cfg.step + 2, np.int32)
    want_live[cfg.step], want_live[cfg.step + 1] = cfg.live, int(f32["live_next"])
    np.testing.assert_array_equal(live[:-1], want_live, err_msg="live " + what)
    for k in ("stop", "digits"):
        sentinel_intact(t[k], B, f"{k} {what}")
    sentinel_intact(t["live"], cfg.step + 2, "live " + what)
    for k, (a, h) in enumerate(zip(hid_in, t["hid"])):
        if h is None:
            continue
        sentinel_intact(h, B * R.HS, f"hid[{k}] rows >= B {what}")
        got = host(h)[:B * R.HS].reshape(B, R.HS)
        if k < 6:
            assert_bits(got, a, f"hid[{k}] is an input {what}")
        else:  # the finished relu activations
            assert_bits(got, f32["fin"][k - 6], f"hid[{k}] finished {what}")
            cols.add(f"hid[{k}]", got, f64["fin"][k - 6], r32["fin"][k - 6])
            edge = inp["raw"][k - 6][:, list(R.RELU_EDGE_UNITS)]
            ge = got[:, list(R.RELU_EDGE_UNITS)]
            assert (ge[edge <= F(-0.5)] == 0).all() and (ge[edge > F(-0.5)] > 0).all()
    return t, f64


@pytest.mark.parametrize("ci", range(len(STEP_CFGS)))
@pytest.mark.parametrize("learned", [False, True], ids=["fixed", "learned"])
def test_step_forward(learned, ci):
    """Every output bit-exact against step_fwd_f32 and within the bound against
    step_ref, over the per-image case table (asr_cell_ref.STEP_ROWS) in launches
    of B = 1, 4, 5 and 7 images; rows >= B of every buffer untouched.  A column
    is one output over all these launches.
    Worst ratio against the bound: 0.512 (rec[skl]), MI355X, 2026-10-21."""
    cfg = STEP_CFGS[ci]
    cols = Columns()
    seen = set()
    for B in STEP_B:
        for off in _offsets(B):
            inp = R.step_case(B, off, 100 * ci + 10 * B + off, cfg, learned)
            _, f64 = _check_step_forward(inp, cfg, learned, cols, f"cfg {ci} B={B} off={off}")
            seen |= set(zip(f64["rec"][Q["act_old"]], f64["rec"][Q["act"]]))
    assert seen == {(1.0, 1.0), (1.0, 0.0), (0.0, 0.0)}, seen
    cols.check(f"step forward cfg {ci} learned={learned}")


def _run_step_backward(t, inp, cfg, learned, cot):
    ops = torch.ops.mog_air
    B = len(inp["stop_old"])
    dn = 14 if learned else 12
    douts = nan_buf(B * dn, dn)
    dpre = [None if h is None else nan_buf(B * R.HS, R.HS) for h in t["hid"]]
    ops.asr_step_backward_(B, cfg.train, cfg.fix_steps, cfg.temperature, cfg.gcm, cfg.gcvar,
                           cot["grad_scale"], t["w"], t["gw"], t["hid"], t["rec"], t["eps_shift"],
                           t["eps_scale"], dev(cot["dtheta_fwd"]), dev(cot["dtheta_back"]),
                           dev(cot["dot"]), dev(cot["dreg"]), dev(cot["dss"]), douts, dpre)
    sentinel_intact(douts, B * dn, "douts")
    for k, d in enumerate(dpre):
        if d is not None:
            sentinel_intact(d, B * R.HS, f"dpre[{k}]")
    return (host(douts)[:B * dn].reshape(B, dn),
            [None if d is None else host(d)[:B * R.HS].reshape(B, R.HS) for d in dpre])


@pytest.mark.parametrize("ci", range(len(STEP_CFGS)))
@pytest.mark.parametrize("learned", [False, True], ids=["fixed", "learned"])
def test_step_backward(learned, ci):
    """douts and every dpre[k] against step_ref's autograd, column by column,
    on the record and the finished hidden rows the forward kernel left; exact
    zeros wherever the reference has one (relu masks, act / act_old masks, a
    cotangent that is zero); rows >= B untouched.  Every launch of the case
    table (B = 1, 4, 5, 7) runs with all cotangents together and with each one
    alone (dss given and absent in turn), so that a failure names its term; a
    column is one output over all launches of one cotangent set.
    Worst ratio against the bound: 0.687 (douts[sm1], dtheta_back alone),
    MI355X, 2026-10-21."""
    cfg = STEP_CFGS[ci]
    table = {name: Columns() for name in R.COTANGENTS}
    n = 0
    for B in STEP_B:
        for off in _offsets(B):
            seed = 100 * ci + 10 * B + off
            inp = R.step_case(B, off, seed, cfg, learned)
            t, _, _ = _run_step_forward(inp, cfg, learned)
            n += 1
            for only in R.COTANGENTS:
                cot = R.step_cotangents(B, seed + 1, only=only, dss=(n % 2 == 0 or only == "dss"))
                _, g64 = R.step_ref(inp, cfg, learned, cot)
                _, g32 = R.step_ref(inp, cfg, learned, cot, dtype=torch.float32)
                douts, dpre = _run_step_backward(t, inp, cfg, learned, cot)
                cols = table[only]
                for j in range(douts.shape[1]):
                    cols.add(f"douts[{R.DOUTS[j]}]", douts[:, j], g64["douts"][:, j],
                             g32["douts"][:, j])
                assert len(dpre) == len(g64["dpre"])
                for k, d in enumerate(dpre):
                    assert (d is None) == (g64["dpre"][k] is None), k
                    if d is not None:
                        cols.add(f"dpre[{k}]", d, g64["dpre"][k], g32["dpre"][k])
    for only, cols in table.items():
        cols.check(f"step backward cfg {ci} learned={learned} cotangent={only or 'all'}",
                   exact_zeros=("douts", "dpre"))
