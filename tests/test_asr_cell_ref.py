"""The references of tests/asr_cell_ref.py pinned on the CPU before the GPU
tests trust them: step_ref iterated reproduces oracle.asr_torch.asr_forward,
step_fwd_f32 agrees with it to float32 rounding, the autograd gradients agree
with central finite differences, and three hand-computed tie cases hold TF's
conventions (Maximum: first operand; ReduceMin: even split; the hinge passes
its gradient at 0)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle import asr_oracle as so
from oracle import asr_torch as st
from oracle.air_torch import softplus_tf, transformer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asr_cell_ref as R  # noqa: E402
from asr_cell_ref import Q  # noqa: E402

F = np.float32
OUT_W = ("inf_shift/dense_1", "inf_shift/dense_3", "inf_scale/dense", "inf_scale/dense_1",
         "inf_scale/dense_2", "inf_scale/dense_3", "gen_shift/dense_1", "gen_shift/dense_3",
         "z_pres/prior/dense_1", "z_pres/log_odds/dense_1")


# ------------------------------------------- step_ref inside the model ----
@pytest.mark.parametrize("fix_steps", [None, 2])
def test_step_ref_iterated_reproduces_asr_forward(fix_steps):
    """T = 3 steps, B = 3, every hyper-parameter a float32 value (step_ref
    takes them as the kernels receive them).  The harness recomputes the two
    LSTMCells, the hidden layers and the glimpse VAE as asr_forward does;
    everything between them is step_ref, the terms are terms_ref's function."""
    cfg = so.AsrConfig(batch=3, max_steps=3, z_pres_temperature=0.5, stopping_threshold=0.875,
                       scale_prior_variance=0.0625, fix_steps=fix_steps, constrains_num=(1, 3),
                       constrains_num_gamma=0.5, constrains_margin_gamma=100.0,
                       constrains_num_element_gamma=10.0, constrains_bbox_gamma=1.0,
                       constrains_sharesize_gamma=0.25, constrains_area_gamma=0.125)
    P = {n: torch.tensor(v, dtype=torch.float64)
         for n, v in so.init_params(cfg, seed=31, bias_scale=0.05).items()}
    nz = so.make_noise(cfg, seed=32)
    x, _ = ao.synthetic_canvases(cfg.batch, seed=33)
    images = torch.tensor(x, dtype=torch.float64).reshape(cfg.batch, -1)
    want = st.asr_forward(cfg, P, nz, images)
    B, T, H, Z = cfg.batch, cfg.max_steps, cfg.rnn_units, cfg.vae_latent_dimensions
    C, Wn = cfg.canvas_size, cfg.windows_size
    p = so.P_ROOT
    K = lambda n: P[p + n + "/kernel"]  # noqa: E731
    Bi = lambda n: P[p + n + "/bias"]  # noqa: E731

    def lstm(xin, h, c, scope):
        g = torch.cat([xin, h], 1) @ K(scope) + Bi(scope)
        gi, gj, gf, go = torch.split(g, H, 1)
        c = c * torch.sigmoid(gf + 1.0) + torch.sigmoid(gi) * torch.tanh(gj)
        return torch.tanh(c) * torch.sigmoid(go), c

    def vd(v, name, act=None):
        y = v @ P[p + "vae/" + name + "/weights"] + P[p + "vae/" + name + "/biases"]
        return act(y) if act is not None else y

    w20 = [t.numpy() for n in OUT_W for t in (K(n), Bi(n))]
    z0 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    h, c, hg, cg, hg_prev = (z0(B, H) for _ in range(5))
    zprev, ssprev = z0(B, Z), z0(B, 3)
    stop = np.zeros(B)
    digits = np.zeros(B, np.int32)
    got = {k: [] for k in ("s", "tx", "ty", "zprob", "prn", "kl")}
    steps = 0
    for t in range(T):
        live = bool((stop < cfg.stopping_threshold).any())
        steps += int(live)
        h, c = lstm(torch.cat([images, zprev, ssprev], 1), h, c, "infer_rnn_running")
        hg, cg = lstm(torch.cat([zprev, ssprev], 1), hg, cg, "gen_rnn_running")
        pre = [h @ K("inf_shift/dense") + Bi("inf_shift/dense"),
               h @ K("inf_shift/dense_2") + Bi("inf_shift/dense_2"),
               h @ K("z_pres/log_odds/dense") + Bi("z_pres/log_odds/dense"),
               hg @ K("gen_shift/dense") + Bi("gen_shift/dense"),
               hg @ K("gen_shift/dense_2") + Bi("gen_shift/dense_2"),
               None if fix_steps is not None else
               hg_prev @ K("z_pres/prior/dense") + Bi("z_pres/prior/dense")]
        raw = [h @ K("inf_scale/dense")[:H], h @ K("inf_scale/dense_2")[:H]]
        inp = {"w": w20, "gw": None, "pre": [None if a is None else a.numpy() for a in pre],
               "raw": [a.numpy() for a in raw], "eps_shift": nz["eps_shift"][t],
               "eps_scale": nz["eps_scale"][t], "u": nz["u"][t], "stop_old": stop,
               "digits": digits}
        scfg = R.StepCfg(step=t, train=True, fix_steps=-1 if fix_steps is None else fix_steps,
                         thr=cfg.stopping_threshold, temperature=cfg.z_pres_temperature,
                         gcm=cfg.scale_prior_mean, gcvar=cfg.scale_prior_variance,
                         g_num=cfg.constrains_num_gamma, live=int(live))
        f, _ = R.step_ref(inp, scfg, False)
        rec = f["rec"]
        # the glimpse VAE on this step's theta (its latent feeds the next LSTM input)
        th = torch.tensor(f["theta_fwd"])
        g = transformer(images.view(B, C, C), th, (Wn, Wn)).reshape(B, Wn * Wn)
        a2 = vd(vd(g, "recognition_1", softplus_tf), "recognition_2", softplus_tf)
        mu, lv = vd(a2, "rec_mean"), vd(a2, "rec_log_variance")
        zl = mu + torch.tensor(nz["eps_z"][t], dtype=torch.float64) * torch.sqrt(torch.exp(lv))
        vkl = 0.5 * ((((np.log(cfg.vae_prior_variance) - lv) - 1.0) +
                      torch.exp(lv) / cfg.vae_prior_variance) +
                     (mu - cfg.vae_prior_mean) ** 2 / cfg.vae_prior_variance).sum(1).numpy()
        lw = 1.0 if live else 0.0
        kl = (rec[Q["zkl"]] + rec[Q["skl"]] + rec[Q["shkl"]] + f["zmask"] * vkl) * lw
        for k, v in (("s", rec[Q["s"]]), ("tx", rec[Q["tx"]]), ("ty", rec[Q["ty"]]),
                     ("zprob", rec[Q["zprob"]]), ("prn", rec[Q["prn"]]), ("kl", kl)):
            got[k].append(v)
        np.testing.assert_array_equal(f["scale"], rec[Q["s"]])
        np.testing.assert_array_equal(f["ss"][:, 2], rec[Q["cl"]])
        stop, digits = f["stop"], f["digits"]
        zprev, ssprev, hg_prev = zl, torch.tensor(f["ss"]), hg
    assert steps == want["T"] == 3
    S = {k: np.stack(v[:steps], 1) for k, v in got.items()}
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(S["s"], want["scale"].numpy(), **tol)
    np.testing.assert_allclose(np.stack([S["tx"], S["ty"]], 2), want["shift"].numpy(), **tol)
    np.testing.assert_allclose(S["zprob"], want["z_pres_prob"].numpy(), **tol)
    np.testing.assert_allclose(S["kl"].sum(1), want["kl"].numpy(), **tol)
    np.testing.assert_array_equal(digits, want["digits"].numpy())
    tt = lambda a: torch.tensor(a)  # noqa: E731
    terms = st.structural_terms(cfg, tt(S["s"]), tt(np.stack([S["tx"], S["ty"]], 2)),
                                tt(S["zprob"]), tt(S["prn"]))
    np.testing.assert_allclose(terms["pr"].numpy(), want["pr"].numpy(), **tol)
    act = np.stack(got["kl"]) != 0
    assert act.any() and not act.all()  # some image stopped on the way


# -------------------------------------------------- float32 restatement ----
STEP_CFGS = [R.StepCfg(), R.StepCfg(step=2, fix_steps=2, temperature=1.0, g_num=0.0),
             R.StepCfg(step=2, train=False, fix_steps=3, live=0)]


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("ci", range(len(STEP_CFGS)))
def test_step_fwd_f32_agrees_with_step_ref(ci, learned):
    """Per output column |f32 - f64| <= 2^-16 max(1, max|f64|): the longest
    float32 path is a 66-term fma chain (66 roundings of 2^-24 relative to the
    sum of the terms' magnitudes, a few times the result here), then a dozen
    scalar operations.  Measured worst 0.053 of the bound."""
    cfg = STEP_CFGS[ci]
    worst = 0.0
    for off in (0, 7):
        inp = R.step_case(7, off, 40 + ci, cfg, learned)
        f64, _ = R.step_ref(inp, cfg, learned)
        f32 = R.step_fwd_f32(inp, cfg, learned)
        cols = [(k, f32[k], f64[k]) for k in ("theta_fwd", "theta_back", "ss", "scale", "shift",
                                              "zprob", "zval", "zc", "stop")]
        cols += [(n, f32["rec"][i], f64["rec"][i]) for n, i in Q.items() if i < len(f64["rec"])]
        cols += [(f"hid{6 + k}", a, b) for k, (a, b) in enumerate(zip(f32["fin"], f64["fin"]))]
        for name, a, b in cols:
            lim = 2.0 ** -16 * max(1.0, float(np.abs(b).max()))
            err = float(np.abs(a.astype(np.float64) - b).max())
            worst = max(worst, err / lim)
            assert err <= lim, (name, off, err, lim)
        for k in ("zmask", "digits"):
            np.testing.assert_array_equal(f32[k], f64[k], err_msg=k)
        assert f32["live_next"] == f64["live_next"]
    print(f"cfg {ci} learned={learned}: worst |f32 - f64| / bound = {worst:.3f}")


# ----------------------------------------------------- finite differences ----
FD_H = 1e-5
FD_BOUND = 1e-6


def _fd_check(f, x, g, mask, rng, what):
    """<g, v> against (f(x + h v) - f(x - h v)) / 2h per image, v random on mask."""
    v = rng.standard_normal(x.shape) * mask
    num = (f(x + FD_H * v) - f(x - FD_H * v)) / (2 * FD_H)
    ana = (g * v).reshape(num.shape[0], -1).sum(1) if num.ndim else (g * v).sum()
    scale = np.abs(g * v).reshape(max(num.shape[0], 1) if num.ndim else 1, -1).sum(1) + 1e-3
    rel = float(np.max(np.abs(num - ana) / scale))
    print(f"{what}: FD vs autograd {rel:.2e}")
    assert rel <= FD_BOUND, (what, rel)
    return rel


def test_terms_ref_gradient_vs_finite_differences():
    """Central differences, h = 1e-5 on s, tx, ty, lo (all O(1)): truncation
    h^2 f''' / 6 with f''' up to 1e3 f' (g_margin = 100, the logits of
    probabilities near 0 and 1) is 2e-8 relative, rounding 2^-53 |L| / h with
    |L| up to 1e4 is 1e-7 absolute against sum |g v| of O(100): the bound is
    1e-6 relative to sum |g v|.  Random records sit off every hinge by far more
    than h.  Measured 7e-12."""
    rng = np.random.default_rng(0)
    tb = R.terms_random(5, 3, 3, seed=21)
    cfg = R.loss_cfg(cons=(1, 3))
    gs = 1.0 / 64
    ref = R.terms_ref(tb["rec"], tb["vkl"], tb["zmask"], tb["live"], cfg, grad_scale=gs)
    x = np.stack([tb["rec"][:, Q[k]] for k in ("s", "tx", "ty", "lo")], 1).astype(np.float64)

    def f(xx):
        s, tx, ty, lo = (torch.tensor(xx[:, k].T) for k in range(4))
        zp = torch.sigmoid(lo)
        prn = (zp * softplus_tf(-lo) + (1.0 - zp) * softplus_tf(lo)) * cfg.constrains_num_gamma
        g = st.structural_terms(cfg, s, torch.stack([tx, ty], 2), zp, prn)
        return np.float64(gs * (g["pr"] + g["element"]).sum() + g["margin"])

    _fd_check(f, x, ref["dreg"], np.ones_like(x), rng, "terms_ref")


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("ci", range(len(STEP_CFGS)))
def test_step_ref_gradients_vs_finite_differences(ci, learned):
    """dpre[k] by a random direction per image over the units away from the
    relu edge (|pre-activation| >= 1e-3; the step is 1e-6); douts by
    perturbing the output layers' biases, which shifts exactly the value each
    douts column differentiates.  L is separable over images, so one
    perturbed evaluation gives every image's derivative.  h = 1e-5: truncation
    h^2 f''' / 6 with f''' up to 1 / temperature^3 = 1e3 times f' is 2e-8
    relative, rounding 2^-53 |L| / h with |L| up to 2e3 (the z_pres KL at |lo| =
    100, exp(clv) / gcvar at clv = 5) is 2e-8 absolute against sum |g v| of
    O(0.1) or more: the bound is 1e-6 relative.  Measured worst 7.1e-8 (dpre[7];
    h = 1e-6 measured 8.9e-7 on dpre[8], all of it rounding)."""
    cfg = STEP_CFGS[ci]
    rng = np.random.default_rng(ci)
    B = 7
    inp = R.step_case(B, 3 * ci, 50 + ci, cfg, learned)
    cot = R.step_cotangents(B, 60 + ci)
    _, g = R.step_ref(inp, cfg, learned, cot)

    def L(**repl):
        vals, _, _ = R._step_graph({**inp, **repl}, cfg, learned, torch.float64)
        return R.step_loss(vals, cot).detach().numpy()

    for k in range(6):
        if inp["pre"][k] is None:
            assert g["dpre"][k] is None
            continue
        x = inp["pre"][k].astype(np.float64)
        f = lambda xx, k=k: L(pre=inp["pre"][:k] + [xx] + inp["pre"][k + 1:])  # noqa: E731
        _fd_check(f, x, g["dpre"][k], np.abs(x) >= 1e-3, rng, f"dpre[{k}]")
        assert (g["dpre"][k][x <= 0] == 0).all()
    for k in range(4 if learned else 2):
        x = inp["raw"][k].astype(np.float64)
        mask = np.ones_like(x)
        mask[:, list(R.RELU_EDGE_UNITS)] = 0
        f = lambda xx, k=k: L(raw=inp["raw"][:k] + [xx] + inp["raw"][k + 1:])  # noqa: E731
        _fd_check(f, x, g["dpre"][6 + k], mask, rng, f"dpre[{6 + k}]")
        # the edge units: pre-activation 0 and just below it are masked, just above passes
        edge = inp["raw"][k][:, list(R.RELU_EDGE_UNITS)]
        ge = g["dpre"][6 + k][:, list(R.RELU_EDGE_UNITS)]
        assert (ge[edge <= F(-0.5)] == 0).all()
    bias_of = {"sm0": ("w", R.B_IS1, 0), "sm1": ("w", R.B_IS1, 1), "slv0": ("w", R.B_IS3, 0),
               "slv1": ("w", R.B_IS3, 1), "lo": ("w", R.B_ZL1, 0), "gsm0": ("w", R.B_GS1, 0),
               "gsm1": ("w", R.B_GS1, 1), "gslv0": ("w", R.B_GS3, 0), "gslv1": ("w", R.B_GS3, 1),
               "plo": ("w", R.B_ZP1, 0), "cm": ("w", R.B_IC1, 0), "clv": ("w", R.B_IC3, 0),
               "gcm": ("gw", R.B_GC1, 0), "gclv": ("gw", R.B_GC3, 0)}
    for col, name in enumerate(R.DOUTS[:g["douts"].shape[1]]):
        key, wi, j = bias_of[name]
        if name == "plo" and cfg.fix_steps >= 0:
            assert (g["douts"][:, col] == 0).all()
            continue

        def f(d, key=key, wi=wi, j=j):
            ws = [np.asarray(a, np.float64).copy() for a in inp[key]]
            ws[wi][j] += d
            return L(**{key: ws})

        num = (f(FD_H) - f(-FD_H)) / (2 * FD_H)
        ana = g["douts"][:, col]
        rel = float(np.max(np.abs(num - ana) / (np.abs(ana) + 1.0)))
        print(f"douts[{name}]: FD vs autograd {rel:.2e}")
        assert rel <= FD_BOUND, (name, rel)


# -------------------------------------------------- hand-computed ties ----
def _one_image(steps, lo=None):
    """rec [T, 30, 1] from per-step (s, tx, ty) and log-odds."""
    T = len(steps)
    rec = np.zeros((T, R.NQ, 1), F)
    for t, (s, tx, ty) in enumerate(steps):
        rec[t, Q["s"], 0], rec[t, Q["tx"], 0], rec[t, Q["ty"], 0] = s, tx, ty
        rec[t, Q["lo"], 0] = 0.0 if lo is None else lo[t]
    rec[:, Q["zprob"]] = 1.0 / (1.0 + np.exp(-rec[:, Q["lo"]].astype(np.float64)))
    z = np.zeros((T, 1), F)
    return rec, z, z, np.ones(T + 1, np.int32)


def test_tie_a_overlap_gradient_goes_to_x():
    """Two boxes sc = 18.75 at (25, 25) and (31.25, 31.25): |dx| = |dy| = 6.25,
    overlap active (smean - md = 12.5, both ordered pairs: over = 25).  TF's
    Maximum gives the tie to its first operand |dx|: d over / d cx0 = +2,
    d cx / d tx = 25, so dreg tx = +-50, ty = 0; d over / d sc = 2 * 0.5 each,
    d sc / d s = 50.  (torch.maximum would give 25 to x and 25 to y.)"""
    cfg = R.loss_cfg(g_num=0, g_margin=0, g_element=0, g_bbox=1, g_size=0, g_area=0)
    rec, vkl, zm, live = _one_image([(0.375, 0.0, 0.0), (0.375, 0.25, 0.25)])
    r = R.terms_ref(rec, vkl, zm, live, cfg, grad_scale=1.0)
    assert r["overlap"][0] == 25.0 and r["out"][0] == 0.0
    np.testing.assert_array_equal(r["dreg"][0, :, 0], [50.0, 50.0, 0.0, 0.0])
    np.testing.assert_array_equal(r["dreg"][1, :, 0], [50.0, -50.0, 0.0, 0.0])


def test_tie_b_reduce_min_splits_evenly():
    """cons = (1, 2), Tx = 2, both z_pres probabilities 0.5 (lo = 0): logit8 is
    exactly 0, the two objectives' cross-entropy sums tie (2 ln 2 each).  TF's
    ReduceMin gives each half: step 1 gets 0.5 (0.5 - 1) + 0.5 (0.5 - 0) = 0,
    step 0 the full (sigmoid(0) - 1) g_element = -5 times d logit8 / d lo =
    0.25 * 2 / (0.5 + 1e-8) = 1 / (1 + 2e-8): -4.9999999000000020.  The margin's
    own gradient does not scale with grad_scale, so the element part is
    dreg(grad_scale = 1) - dreg(grad_scale = 0).  (torch's min(dim) would give
    step 1 -5 or +5.)"""
    cfg = R.loss_cfg(cons=(1, 2), g_num=0, g_margin=100, g_element=10, g_bbox=0, g_size=0,
                     g_area=0)
    rec, vkl, zm, live = _one_image([(0.375, -0.5, 0.0), (0.375, 0.5, 0.0)], lo=(0.0, 0.0))
    r1 = R.terms_ref(rec, vkl, zm, live, cfg, grad_scale=1.0)
    r0 = R.terms_ref(rec, vkl, zm, live, cfg, grad_scale=0.0)
    assert r1["element"][0] == pytest.approx(10 * 2 * 0.6931471805599453, rel=1e-15)
    d = r1["dreg"] - r0["dreg"]
    assert d[1, 3, 0] == 0.0
    assert d[0, 3, 0] == pytest.approx(-4.9999999000000020, abs=1e-12)
    assert (d[:, :3] == 0).all()


def test_tie_c_area_hinge_passes_at_the_bound():
    """One step, sc = 0.5 * 50 = area_max = 25 exactly.  max(area_max - sc, 0)
    passes -1 at equality (tf.maximum(x, 0) and torch.clamp alike); with
    area_min = 30 above sc the other hinge is off: d area / d s = -1 * 50.
    With area_min = 12.5 below, its +1 cancels: exactly 0 (50 if the -1 were
    dropped)."""
    rec, vkl, zm, live = _one_image([(0.5, 0.0, 0.0)])
    base = dict(g_num=0, g_margin=0, g_element=0, g_bbox=0, g_size=0, g_area=1)
    r = R.terms_ref(rec, vkl, zm, live, R.loss_cfg(area_minmax=(30.0, 25.0), **base))
    assert r["area"][0] == 0.0
    np.testing.assert_array_equal(r["dreg"][0, :, 0], [-50.0, 0.0, 0.0, 0.0])
    r = R.terms_ref(rec, vkl, zm, live, R.loss_cfg(area_minmax=(12.5, 25.0), **base))
    assert r["area"][0] == 12.5
    np.testing.assert_array_equal(r["dreg"][0, :, 0], [0.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------- the case tables ----
def test_branch_table_sits_on_its_branches():
    """The geometry rows hit what their comments say, identically in float32
    and float64, and the float32 restatement agrees with terms_ref."""
    tb = R.terms_branch_table()
    rec = tb["rec"]
    for dt in (np.float32, np.float64):
        s = rec[:, Q["s"]].astype(dt)
        sc = s * dt(50)
        cx = (rec[:, Q["tx"]].astype(dt) + dt(1)) * dt(50) / dt(2)
        lo, hi = (dt(v) for v in R.BRANCH_AREA)
        assert (sc == lo).any() and (sc == hi).any() and (sc < lo).any() and (sc > hi).any()
        assert (cx - sc / 2 == 0).any() and (cx + sc / 2 == 50).any()
        assert (cx - sc / 2 < 0).any() and (cx + sc / 2 > 50).any()
        d = np.abs(sc[0] - sc[1])
        assert ((d > 0) & (d < 3)).any() and (d > 3).any() and (d == 0).any()
        assert (d == 3).any() if dt is np.float32 else ((d > 3) & (d < 3 + 1e-5)).any()
    assert (rec[:, Q["zprob"]] == 0.5).any() and (rec[:, Q["zprob"]] < 2e-7).any()
    assert (rec[:, Q["zprob"]] >= 1 - 2.0 ** -23).any()
    for cons in R.BRANCH_CONS:
        cfg = R.loss_cfg(cons=cons, area_minmax=R.BRANCH_AREA)
        r64 = R.terms_ref(rec, tb["vkl"], tb["zmask"], tb["live"], cfg, grad_scale=1 / 64)
        r32 = R.terms_fwd_f32(rec, tb["live"], cfg)
        for k in ("area", "out", "size", "overlap", "element"):
            np.testing.assert_allclose(r32[k], r64[k], rtol=1e-5, atol=1e-5, err_msg=k)
        assert (r64["dreg"] == 0).any() and np.isfinite(r64["dreg"]).all()
