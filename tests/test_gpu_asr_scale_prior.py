"""AIR-ASR learned scale prior (fix_scale_distribution=False) on the GPU: the
learned variants of the step kernels (asr_cell.hip, asr_gen.hip) through
mog_air.asr_model.AIRModel against the fixed-prior C oracle where the flag
changes nothing (everything but scale_kls and the loss, bit for bit), against
the numpy restatement (tests/asr_scale_prior_ref.py) for the scale KL and the
generation loop, and against float64 autograd of the torch restatement for
the gradients; eager and captured train steps, and the entry point."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import asr_oracle as so

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asr_gen_ref as gref  # noqa: E402
import asr_scale_prior_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, P, scope, precision="fp32", learned=True, **kw):
    from mog_air.asr_model import AIRModel
    m = AIRModel(max_steps=cfg.max_steps, max_digits=cfg.max_steps, canvas_size=cfg.canvas_size,
                 fix_scale_distribution=not learned,
                 vae_likelihood_std=cfg.vae_likelihood_std, z_pres_prior_log_odds=-0.01,
                 z_pres_temperature=cfg.z_pres_temperature,
                 stopping_threshold=cfg.stopping_threshold, learning_rate=1e-4,
                 gradient_clipping_norm=1.0, cnn=False, train=cfg.train, scope=scope,
                 constrains_num=list(cfg.constrains_num),
                 constrains_num_gamma=cfg.constrains_num_gamma,
                 constrains_margin_gamma=cfg.constrains_margin_gamma,
                 constrains_num_element_gamma=cfg.constrains_num_element_gamma,
                 constrains_bbox_gamma=cfg.constrains_bbox_gamma,
                 constrains_sharesize_gamma=cfg.constrains_sharesize_gamma,
                 constrains_area_gamma=cfg.constrains_area_gamma,
                 constrains_area_minmax=list(cfg.constrains_area_minmax),
                 fix_steps=cfg.fix_steps, device=DEV, precision=precision, **kw)
    assert m.fix_scale_distribution is (not learned)
    if P is not None:
        m.params.load_dict(P)
    return m


def _noise(nz):
    return {n: torch.as_tensor(np.array(v)).to(DEV) for n, v in nz.items()}


def _outputs(m):
    """Everything the flag must leave alone."""
    ws = m._ws
    out = {"digits": m.rec_num_digits, "scale": m.rec_scales, "shift": m.rec_shifts,
           "zprob": m.z_pres_probs, "zkl": m.z_pres_kls, "shkl": m.shift_kls, "vkl": m.vae_kls,
           "windows": m.rec_windows, "canvas": m.canvas, "area": ws.area, "out": ws.outl,
           "size": ws.size, "overlap": ws.over, "element": ws.element, "pr": ws.pr}
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


# ------------------------------------------------------------ forward ----
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("fix", [None, 2])
@pytest.mark.parametrize("k", sorted(ref.SETS))
def test_forward_fp32_flag_moves_only_the_scale_kl(k, fix, train, fused):
    ref.check_case(ref.case(k))
    c = ref.case(k, fix_steps=fix, train=train)
    cfg, o, want = c["cfg"], c["ref"], c["learned"]
    m = _model(cfg, c["P"], f"lsf{k}{fix}{train}{fused}")
    if fused:
        m.FUSED_F32_MIN_ROWS = 0
    m.infer(c["x"], c["tg"], noise=_noise(c["nz"]))
    assert m.executed_steps == o["T"]
    got = _outputs(m)
    for key, w in (("digits", o["digits"]), ("scale", o["scale"].T[..., None]),
                   ("shift", o["shift"].transpose(1, 0, 2)), ("zprob", o["z_pres_prob"].T),
                   ("zkl", o["z_pres_kl"].T), ("shkl", o["shift_kl"].T), ("vkl", o["vae_kl"].T),
                   ("windows", o["window"].transpose(1, 0, 2)), ("canvas", o["canvas"]),
                   ("area", o["area"]), ("out", o["out"]), ("size", o["size"]),
                   ("overlap", o["overlap"]), ("element", o["element"]), ("pr", o["pr_loss"])):
        np.testing.assert_array_equal(got[key], w, err_msg=key)
    skl = m.scale_kls.cpu().numpy()
    np.testing.assert_array_equal(skl, want["scale_kl"].T)
    assert np.any(skl != o["scale_kl"].T)
    loss = (o["loss"] - o["scale_kl"].sum(0)) + want["scale_kl"].sum(0)
    np.testing.assert_allclose(m.per_image_loss.cpu().numpy(), loss, rtol=1e-5)
    assert np.isfinite(m.log_variables["scale_kl"])


# ------------------------------------------------- bf16 trajectory -------
def test_bf16_trajectory_is_the_fixed_prior_one():
    c = ref.case(1)
    ref.check_case(c)
    cfg = c["cfg"]
    ml = _model(cfg, c["P"], "lsb_l", "bf16")
    mf = _model(cfg, c["P_fixed"], "lsb_f", "bf16", learned=False)
    for n in c["P_fixed"]:
        assert torch.equal(ml.params.view(n), mf.params.view(n)), n
    nz = _noise(c["nz"])
    ml.infer(c["x"], c["tg"], noise=nz)
    mf.infer(c["x"], c["tg"], noise=nz)
    a, b = _outputs(ml), _outputs(mf)
    T = ml.executed_steps
    assert T == mf.executed_steps and T >= 2
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    # the scale KL from the model's own device records through the helper's heads
    from mog_air.asr_model import Q
    rec = ml._ws.arec.cpu().numpy()
    hg = ml._ws.hg.cpu().numpy()
    want = []
    for t in range(T):
        r = rec[t]
        sl = np.ascontiguousarray(np.stack([r[Q["sl0"]], r[Q["sl1"]]], axis=1))
        act = r[Q["act"]] != 0
        want.append(ref.learned_scale_kl(c["P"], hg[t], sl, r[Q["cm"]].copy(),
                                         r[Q["clv"]].copy(), act))
        assert act.any() or t > 0
    want = np.stack(want, axis=1)
    got = ml.scale_kls.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert np.any(got != mf.scale_kls.cpu().numpy())


# ---------------------------------------------------- degenerate prior ----
def test_zero_gen_scale_heads_give_the_fixed_prior():
    c = ref.case(2)
    ref.check_case(c)
    cfg = c["cfg"]
    P = dict(c["P"])
    for n, shape in ref.gen_scale_specs(cfg):
        P[n] = np.zeros(shape, np.float32)
    P[so.P_ROOT + "gen_scale/dense_1/bias"] = np.array([-1.0], np.float32)
    P[so.P_ROOT + "gen_scale/dense_3/bias"] = np.array([np.log(np.float32(0.05))], np.float32)
    ml = _model(cfg, P, "lsd_l")
    mf = _model(cfg, c["P_fixed"], "lsd_f", learned=False)
    nz = _noise(c["nz"])
    ml.infer(c["x"], c["tg"], noise=nz)
    mf.infer(c["x"], c["tg"], noise=nz)
    a, b = ml.scale_kls.cpu().numpy(), mf.scale_kls.cpu().numpy()
    assert np.any(b != 0)
    np.testing.assert_allclose(a, b, rtol=1e-6)
    assert ml.loss == pytest.approx(mf.loss, rel=1e-5)


# ------------------------------------------------------------ gradients ---
def _f64_grads(c, learned, P=None, scale=None):
    cfg = c["cfg"]
    P = c["P"] if P is None else P
    Pt = {n: torch.tensor(v if scale is None else scale(n, v), dtype=torch.float64,
                          requires_grad=True) for n, v in P.items()}
    x = torch.tensor(np.array(c["x"]), dtype=torch.float64).reshape(cfg.batch, -1)
    out = ref.asr_loss_torch(cfg, Pt, c["nz"], x, torch.tensor(c["Gc"], dtype=torch.float64),
                             learned)
    out["loss"].backward()
    return {n: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape))
            for n, p in Pt.items()}


def _gradient_case(k, fix):
    c = dict(ref.case(k, fix_steps=fix))
    cfg = c["cfg"]
    c["Gc"] = (np.random.default_rng(31).standard_normal((cfg.batch, cfg.canvas_size ** 2)) *
               0.01).astype(np.float32)
    return c


def _check_gradients(c, grads, want, tol, cos_min, global_tol, conditioned, min_checked):
    checked, worst = 0, 0.0
    got_all, ref_all = [], []
    for name, r in want.items():
        g = np.asarray(grads[name], np.float64)
        got_all.append(g.ravel())
        ref_all.append(r.ravel())
        if np.linalg.norm(r) < 1e-6:
            assert np.linalg.norm(g) < 1e-4, name
            continue
        err = np.linalg.norm(g - r) / np.linalg.norm(r)
        cos = float(np.dot(g.ravel(), r.ravel()) / (np.linalg.norm(g) * np.linalg.norm(r) + 1e-30))
        print(f"{name}: rel {err:.3e} cos {cos:.6f} conditioned {conditioned[name]}")
        if not conditioned[name]:
            continue
        worst = max(worst, err)
        checked += 1
        assert err < tol and cos > cos_min, (name, err, cos)
    g, r = np.concatenate(got_all), np.concatenate(ref_all)
    gerr = np.linalg.norm(g - r) / np.linalg.norm(r)
    gcos = float(np.dot(g, r) / (np.linalg.norm(g) * np.linalg.norm(r)))
    print(f"worst checked {worst:.3e}, global {gerr:.3e} cos {gcos:.6f}, checked {checked}")
    assert gerr < global_tol and gcos > 0.99, (gerr, gcos)
    assert checked >= min_checked


@pytest.mark.parametrize("fix", [None, 2])
@pytest.mark.parametrize("k", sorted(ref.SETS))
def test_gradients_fp32_vs_float64_autograd(k, fix):
    ref.check_case(ref.case(k))
    c = _gradient_case(k, fix)
    cfg = c["cfg"]
    nz, Gc = _noise(c["nz"]), torch.as_tensor(c["Gc"]).to(DEV)
    m = _model(cfg, c["P"], f"lsg{k}{fix}")
    grads = m.compute_gradients(c["x"], c["tg"], noise=nz, canvas_cotangent=Gc)
    want = _f64_grads(c, True)
    assert set(grads) == set(want)
    _check_gradients(c, grads, want, 2e-3, 0.999, 2e-3, {n: True for n in want}, 40)
    for n, _ in ref.gen_scale_specs(cfg):
        assert np.abs(grads[n]).max() > 0, n
    assert np.abs(grads[so.P_ROOT + "gen_rnn_running/kernel"]).max() > 0
    # against the fixed prior on the same weights: through the shift latent the
    # prior's gradient reaches the inference shift heads and both LSTMCells.
    # The gen_shift heads' own gradient is hg^T d(shift KL): the flag moves no
    # forward value, so it stays what it was (float64 autograd agrees, see
    # test_asr_scale_prior.py) -- checked here as equality within the fp32 gate
    mf = _model(cfg, c["P_fixed"], f"lsg{k}{fix}f", learned=False)
    gf = mf.compute_gradients(c["x"], c["tg"], noise=nz, canvas_cotangent=Gc)
    for n in ("inf_shift/dense/kernel", "inf_shift/dense_2/kernel", "gen_rnn_running/kernel",
              "infer_rnn_running/kernel"):
        n = so.P_ROOT + n
        assert np.linalg.norm(grads[n] - gf[n]) > 1e-3 * np.linalg.norm(gf[n]), n
    for n in gf:
        if "/gen_shift/" in n:
            np.testing.assert_allclose(grads[n], gf[n], rtol=0, atol=2e-3 * np.abs(gf[n]).max())


def test_gradients_bf16_vs_float64_autograd():
    """The gates of tests/test_gpu_asr.py's bf16 row: tensors whose float64
    gradient moves < 10 % under a 0.4 % perturbation of the VAE weights within
    20 %, cosine >= 0.99; the whole gradient within 8 %; >= 40 checked."""
    ref.check_case(ref.case(1))
    c = _gradient_case(1, None)
    cfg = c["cfg"]
    m = _model(cfg, c["P"], "lsgb", "bf16")
    grads = m.compute_gradients(c["x"], c["tg"], noise=_noise(c["nz"]),
                                canvas_cotangent=torch.as_tensor(c["Gc"]).to(DEV))
    want = _f64_grads(c, True)
    r2 = np.random.default_rng(5)
    pert = _f64_grads(c, True, scale=lambda n, v: v * (1 + 4e-3 * r2.standard_normal(v.shape))
                      if "/vae/" in n else v)
    conditioned = {n: np.linalg.norm(want[n] - pert[n]) < 0.1 * np.linalg.norm(want[n])
                   for n in want}
    _check_gradients(c, grads, want, 2e-1, 0.99, 8e-2, conditioned, 40)


# ---------------------------------------------------------------- graph ---
def test_graph_replay_matches_eager_bitwise():
    import bench
    cfg = ref.case(1)["cfg"]
    me = _model(cfg, None, "lsgr_e", seed=21, noise_seed=22)
    mg = _model(cfg, None, "lsgr_g", seed=21, noise_seed=22)
    assert torch.equal(me.params.flat, mg.params.flat)
    for i in range(3):
        x, k = bench.synthetic(8, 300 + i)
        x, k = torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV)
        me.train_step_async(x, k)
        mg.train_step_graphed(x, k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(me._ws.means[:3].cpu().numpy(),
                                      mg._ws.means[:3].cpu().numpy(), err_msg=f"step {i}")
        assert torch.equal(me.params.grad.view(torch.int32), mg.params.grad.view(torch.int32)), i
        assert torch.equal(me.params.flat.view(torch.int32), mg.params.flat.view(torch.int32)), i
    assert mg._graph is not None
    assert torch.equal(me.params.m.view(torch.int32), mg.params.m.view(torch.int32))
    o = me.params.offsets[so.P_ROOT + "gen_scale/dense/kernel"]
    assert float(me.params.m[o:o + 258 * 64].abs().max()) > 0  # Adam moved the new block


# ----------------------------------------------------------- generation ---
GEN_CASES = {1: (4, 5, None), 2: (4, 17, None), 3: (3, 6, 2)}
_GEN = {}


def _gen_case(k):
    if k not in _GEN:
        T, G, fix = GEN_CASES[k]
        cfg = so.AsrConfig(batch=G, max_steps=T, train=False, z_pres_temperature=1.0,
                           vae_likelihood_std=0.3, stopping_threshold=0.9,
                           constrains_area_minmax=(17.0, 23.0), fix_steps=fix)
        P = so.init_params(cfg, seed=60 + k, bias_scale=0.05)
        P.update(ref.gen_scale_params(cfg, 160 + k, bias_scale=0.05))
        nz = so.make_noise(cfg, seed=70 + k)
        nz["u_x"] = np.random.default_rng(70 + k).uniform(0, 1, (T, G, 784)).astype(np.float32)
        _GEN[k] = (cfg, P, nz, ref.generate(cfg, P, nz, G, True), gref.generate(cfg, P, nz, G))
    return _GEN[k]


@pytest.mark.parametrize("k", sorted(GEN_CASES))
def test_generation_matches_reference(k):
    T, G, fix = GEN_CASES[k]
    cfg, P, nz, out, fixed = _gen_case(k)
    # the reference is not degenerate, and the learned latent reached the LSTM
    assert out["T"] >= 2 and out["canvas"].max() > 0
    n = min(out["T"], fixed["T"])
    assert np.array_equal(out["st_back"][0], fixed["st_back"][0])
    assert any(not np.array_equal(out["st_back"][t], fixed["st_back"][t]) for t in range(1, n))
    from mog_air.asr_model import AIRModel
    kw = dict(max_steps=T, cnn=False, train=False, z_pres_temperature=1.0, vae_likelihood_std=0.3,
              stopping_threshold=0.9, constrains_area_minmax=(17, 23), fix_steps=fix,
              generation_batch_size=G, device=DEV)
    noise = _noise(nz)
    for learned, want in ((True, out), (False, fixed)):
        m = AIRModel(fix_scale_distribution=not learned, scope=f"lsgen{k}{learned}", **kw)
        m.params.load_dict(P)
        canvas = m.generate(noise=noise).reshape(G, -1).cpu().numpy()
        st = m.generated_st_back.cpu().numpy()
        assert st.shape == (G, want["T"], 2, 3)
        np.testing.assert_array_equal(st, want["st_back"].transpose(1, 0, 2).reshape(G, -1, 2, 3))
        np.testing.assert_array_equal(m.generated_num_digits.cpu().numpy(), want["digits"])
        np.testing.assert_array_equal(canvas, want["canvas"])


# ------------------------------------------------------ scope / entry -----
def test_reuse_across_the_flag_is_refused():
    cfg = ref.case(1)["cfg"]
    _model(cfg, None, "lsreuse")
    from mog_air.asr_model import AIRModel
    with pytest.raises(ValueError, match="different variable shapes"):
        AIRModel(max_steps=cfg.max_steps, cnn=False, fix_scale_distribution=True, reuse=True,
                 scope="lsreuse", device=DEV)
    t = AIRModel(max_steps=cfg.max_steps, cnn=False, fix_scale_distribution=False, reuse=True,
                 scope="lsreuse", device=DEV)
    assert t.fix_scale_distribution is False


def test_train_air_pr_learned_scale_prior(tmp_path, monkeypatch):
    import train_air_pr as entry
    from mog_air.asr_model import AIRModel
    monkeypatch.chdir(tmp_path)
    step = entry.main(["-dn", "13", "-gm", "100", "-gne", "10", "-r", str(tmp_path / "res"), "-k",
                       "s", "--learned_scale_prior", "--iterations", "5", "--synth-per-count",
                       "40"])
    assert step == 5
    folder = tmp_path / "res_(s)"
    text = "".join(open(f, errors="ignore").read() for f in glob.glob(str(folder / "*"))
                   if os.path.isfile(f))
    losses = [float(v) for v in re.findall(r"TotLoss:(\S+)", text)]
    assert losses and np.all(np.isfinite(losses))
    ckpt = sorted(glob.glob(str(folder / "models" / "air-model-*.npz")))
    assert ckpt
    saved = {k.replace("__", "/"): v for k, v in np.load(ckpt[-1]).items()}
    names = [n for n, _ in ref.gen_scale_specs(so.AsrConfig())]
    for n in names:
        assert n in saved and np.isfinite(saved[n]).all(), n
    m = AIRModel(max_steps=6, cnn=False, fix_scale_distribution=False, scope="lsckpt", device=DEV,
                 seed=99)
    m.params.load_dict(saved)
    back = m.params.state_dict()
    assert set(back) == set(saved)
    for n in saved:
        assert np.array_equal(back[n].view(np.int32), saved[n].view(np.int32)), n
