"""TEST HELPER (not collected) -- the learned scale prior of AIR-ASR
(fix_scale_distribution=False; air/air_number_bbox_location.py:482-509,
:729-746, :1170-1201) restated from primitives the CPU oracle exports.

Three parts:

* ``scale_kl_numpy``: what the scale KL needs, per loop step in numpy float32
  (``ao.dense_chain`` k-ordered fma chains, ``oracle_math_vec`` transcendentals,
  one rounding per operation like the contraction-off C): both LSTMCells, the
  inf_shift / inf_scale heads with sampling, the gen_scale heads and the masked
  KL against either prior.  The glimpse VAE is not restated: z of each step is
  the oracle's own ``latent`` output, activity comes from its ``z_pres``.
* ``asr_loss_torch``: the whole train loss in torch (float64-capable) with the
  flag, for gradients by autograd.
* ``generate``: the generation loop of tests/asr_gen_ref.py with the scale
  latent drawn from the gen_scale heads.
"""
import numpy as np
import torch

from oracle import air_oracle as ao
from oracle import asr_oracle as so
from oracle.air_torch import concrete_kl, softplus_tf, transformer

import asr_gen_ref as gref
from asr_gen_ref import EXP, LOG, SIGMOID, SOFTPLUS, TANH, _math, _relu

f32 = np.float32
P_ROOT = so.P_ROOT
GEN_SCALE = ("gen_scale/dense", "gen_scale/dense_1", "gen_scale/dense_2", "gen_scale/dense_3")


def gen_scale_specs(cfg):
    H, HS = cfg.rnn_units, cfg.scale_hidden_units
    shapes = ((H + 2, HS), (HS + 2, 1), (H + 2, HS), (HS + 2, 1))
    out = []
    for n, (i, o) in zip(GEN_SCALE, shapes):
        out += [(P_ROOT + n + "/kernel", (i, o)), (P_ROOT + n + "/bias", (o,))]
    return out


def gen_scale_params(cfg, seed, bias_scale=0.0):
    """The eight gen_scale tensors, Glorot-uniform kernels as so.init_params."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in gen_scale_specs(cfg):
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rng.uniform(-lim, lim, size=shape).astype(f32)
        else:
            out[name] = (rng.uniform(-bias_scale, bias_scale, size=shape).astype(f32)
                         if bias_scale > 0 else np.zeros(shape, f32))
    return out


# ------------------------------------------------------------- numpy -----
def _p(P, n):
    return np.ascontiguousarray(P[P_ROOT + n], f32)


def _lstm(P, scope, x, h, c, H):
    gates = ao.dense_chain(np.concatenate([x, h], axis=1), _p(P, scope + "/kernel"),
                           _p(P, scope + "/bias"))
    gi, gj, gf, go = (gates[:, k * H:(k + 1) * H] for k in range(4))
    c = c * _math(SIGMOID, gf + f32(1)) + _math(SIGMOID, gi) * _math(TANH, gj)
    return _math(TANH, c) * _math(SIGMOID, go), c


def scale_heads(P, scope, h, sl):
    """mean, log-variance [B] of the inf_scale / gen_scale head pair on
    concat([h, sl]): hidden = relu(chain + b), out = chain over concat([hidden,
    sl]) + b."""
    hin = np.concatenate([h, sl], axis=1)
    out = []
    for a, b in (("dense", "dense_1"), ("dense_2", "dense_3")):
        hid = _relu(ao.dense_chain(hin, _p(P, scope + "/" + a + "/kernel"),
                                   _p(P, scope + "/" + a + "/bias")))
        out.append(ao.dense_chain(np.concatenate([hid, sl], axis=1),
                                  _p(P, scope + "/" + b + "/kernel"),
                                  _p(P, scope + "/" + b + "/bias"))[:, 0])
    return out


def gaussian_kl(cm, clv, gcm, gclv, gcvar, act):
    """0.5 ((((gclv - clv) - 1) + cvar / gcvar) + dc dc / gcvar), masked."""
    cvar = _math(EXP, clv)
    dc = cm - gcm
    skl = f32(0.5) * ((((gclv - clv) - f32(1)) + cvar / gcvar) + (dc * dc) / gcvar)
    assert skl.dtype == f32
    return np.where(act, skl, f32(0)).astype(f32)


def learned_scale_kl(P, hg, sl, cm, clv, act):
    """The scale KL against the gen_scale heads' Gaussian on (hg, sl)."""
    gcm, gclv = scale_heads(P, "gen_scale", hg, sl)
    return gaussian_kl(cm, clv, gcm, gclv, _math(EXP, gclv), act)


def scale_kl_numpy(cfg, P, noise, images, ref, learned):
    """``ref``: so.forward's result on the same inputs (latent, z_pres, T).
    Returns scale [T,B], shift [T,B,2], scale_kl [T,B], act [T,B] (bool)."""
    B, H, Z = cfg.batch, cfg.rnn_units, cfg.vae_latent_dimensions
    x = np.ascontiguousarray(images, f32).reshape(B, -1)
    nz = {k: np.ascontiguousarray(v, f32) for k, v in noise.items()}
    thr = f32(cfg.stopping_threshold)
    h, c, hg, cg = (np.zeros((B, H), f32) for _ in range(4))
    z_prev, ss_prev = np.zeros((B, Z), f32), np.zeros((B, 3), f32)
    stop = np.zeros(B, f32)
    out = {k: [] for k in ("scale", "shift", "scale_kl", "act")}
    for t in range(ref["T"]):
        h, c = _lstm(P, "infer_rnn_running", np.concatenate([x, z_prev, ss_prev], axis=1), h, c, H)
        hm = _relu(ao.dense_chain(h, _p(P, "inf_shift/dense/kernel"), _p(P, "inf_shift/dense/bias")))
        sm = ao.dense_chain(hm, _p(P, "inf_shift/dense_1/kernel"), _p(P, "inf_shift/dense_1/bias"))
        hv = _relu(ao.dense_chain(h, _p(P, "inf_shift/dense_2/kernel"),
                                  _p(P, "inf_shift/dense_2/bias")))
        slv = ao.dense_chain(hv, _p(P, "inf_shift/dense_3/kernel"), _p(P, "inf_shift/dense_3/bias"))
        sl = sm + nz["eps_shift"][t] * np.sqrt(_math(EXP, slv))
        cm, clv = scale_heads(P, "inf_scale", h, sl)
        cl = cm + nz["eps_scale"][t] * np.sqrt(_math(EXP, clv))
        hg, cg = _lstm(P, "gen_rnn_running", np.concatenate([z_prev, ss_prev], axis=1), hg, cg, H)
        stop = stop + (f32(1) - ref["z_pres"][t])
        act = stop < thr
        if learned:
            skl = learned_scale_kl(P, hg, sl, cm, clv, act)
        else:
            skl = gaussian_kl(cm, clv, f32(cfg.scale_prior_mean),
                              ao.f32log(cfg.scale_prior_variance), f32(cfg.scale_prior_variance),
                              act)
        out["scale"].append(_math(SIGMOID, cl))
        out["shift"].append(_math(TANH, sl))
        out["scale_kl"].append(skl)
        out["act"].append(act)
        z_prev = np.ascontiguousarray(ref["latent"][t], f32)
        ss_prev = np.concatenate([sl, cl[:, None]], axis=1).astype(f32)
        for a in (h, hg, sl, cl, skl):
            assert a.dtype == f32
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------- torch -----
def _sce(z, x):
    return torch.clamp(x, min=0.0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))


def _logit8(p):
    return torch.log(p + 1e-8) - torch.log(1.0 - p + 1e-8)


def asr_loss_torch(cfg, P, noise, images, canvas_cotangent, learned):
    """The train loss of air_number_bbox_location.py:384-1079 on the fixed-T
    schedule (steps past the global exit masked), the reconstruction term
    replaced by <canvas_cotangent, canvas> (as oracle.asr_torch does with a
    cotangent), the scale KL against the fixed or the learned prior."""
    dt = images.dtype
    B, T, H, Z = cfg.batch, cfg.max_steps, cfg.rnn_units, cfg.vae_latent_dimensions
    C, W = cfg.canvas_size, cfg.windows_size
    p = P_ROOT

    def dense(x, scope, act=None):
        y = x @ P[p + scope + "/kernel"] + P[p + scope + "/bias"]
        return act(y) if act is not None else y

    def vdense(x, name, act=None):
        y = x @ P[p + "vae/" + name + "/weights"] + P[p + "vae/" + name + "/biases"]
        return act(y) if act is not None else y

    def lstm(x, h, c, scope):
        g = torch.cat([x, h], 1) @ P[p + scope + "/kernel"] + P[p + scope + "/bias"]
        gi, gj, gf, go = torch.split(g, H, 1)
        c = c * torch.sigmoid(gf + 1.0) + torch.sigmoid(gi) * torch.tanh(gj)
        return torch.tanh(c) * torch.sigmoid(go), c

    def pair(hin, sl, scope):
        m = dense(torch.cat([dense(hin, scope + "/dense", torch.relu), sl], 1), scope + "/dense_1")
        v = dense(torch.cat([dense(hin, scope + "/dense_2", torch.relu), sl], 1),
                  scope + "/dense_3")
        return m[:, 0], v[:, 0]

    z0 = lambda *s: torch.zeros(s, dtype=dt)  # noqa: E731
    h, c, hg, cg, hg_prev = (z0(B, H) for _ in range(5))
    zprev, ssprev, stop, canvas = z0(B, Z), z0(B, 3), z0(B), z0(B, C * C)
    f_gclv = float(np.log(np.float32(cfg.scale_prior_variance), dtype=np.float32)) \
        if dt == torch.float32 else float(np.log(cfg.scale_prior_variance))
    vplv = float(np.log(cfg.vae_prior_variance))
    thr, Tq = cfg.stopping_threshold, cfg.z_pres_temperature
    rec = {k: [] for k in ("scale", "shift", "zprob", "kl", "prn")}
    steps = 0
    for t in range(T):
        live = bool((stop < thr).any())
        steps += int(live)
        tn = lambda k: torch.as_tensor(noise[k][t], dtype=dt)  # noqa: E731
        h, c = lstm(torch.cat([images, zprev, ssprev], 1), h, c, "infer_rnn_running")
        sm = dense(dense(h, "inf_shift/dense", torch.relu), "inf_shift/dense_1")
        slv = dense(dense(h, "inf_shift/dense_2", torch.relu), "inf_shift/dense_3")
        svar = torch.exp(slv)
        sl = sm + tn("eps_shift") * torch.sqrt(svar)
        shift = torch.tanh(sl)
        cm, clv = pair(torch.cat([h, sl], 1), sl, "inf_scale")
        cvar = torch.exp(clv)
        cl = cm + tn("eps_scale") * torch.sqrt(cvar)
        s = torch.sigmoid(cl)
        hg, cg = lstm(torch.cat([zprev, ssprev], 1), hg, cg, "gen_rnn_running")
        gsm = dense(dense(hg, "gen_shift/dense", torch.relu), "gen_shift/dense_1")
        gslv = dense(dense(hg, "gen_shift/dense_2", torch.relu), "gen_shift/dense_3")
        if learned:  # (:482-509: the INFERENCE shift latent)
            gcm, gclv = pair(torch.cat([hg, sl], 1), sl, "gen_scale")
            gcvar = torch.exp(gclv)
        else:
            gcm, gclv, gcvar = cfg.scale_prior_mean, f_gclv, cfg.scale_prior_variance
        tx, ty = shift[:, 0], shift[:, 1]
        zr = torch.zeros_like(s)
        g = transformer(images.view(B, C, C), torch.stack([s, zr, tx, zr, s, ty], 1),
                        (W, W)).reshape(B, W * W)
        a2 = vdense(vdense(g, "recognition_1", softplus_tf), "recognition_2", softplus_tf)
        mu, lv = vdense(a2, "rec_mean"), vdense(a2, "rec_log_variance")
        zl = mu + tn("eps_z") * torch.sqrt(torch.exp(lv))
        d2 = vdense(vdense(zl, "generative_1", softplus_tf), "generative_2", softplus_tf)
        r = torch.sigmoid(vdense(d2, "gen_mean") + tn("eps_x") * cfg.vae_likelihood_std)
        thb = torch.stack([1.0 / s, zr, -tx / s, zr, 1.0 / s, -ty / s], 1)
        wr = transformer(r.view(B, W, W), thb, (C, C)).reshape(B, C * C)
        if cfg.fix_steps is not None:
            plo = torch.full((B,), 100.0 if t < cfg.fix_steps else -100.0, dtype=dt)
        else:
            plo = dense(dense(hg_prev, "z_pres/prior/dense", torch.relu),
                        "z_pres/prior/dense_1")[:, 0]
        lo = dense(dense(h, "z_pres/log_odds/dense", torch.relu), "z_pres/log_odds/dense_1")[:, 0]
        u = tn("u")
        y = (lo + (torch.log(u + 1e-9) - torch.log(1.0 - u + 1e-9))) / Tq
        zp = torch.sigmoid(y)
        if not cfg.train:
            zp = torch.round(zp).detach()
        zprob = torch.sigmoid(lo)
        prn = torch.zeros_like(lo)
        if cfg.constrains_num_gamma > 1e-8:
            prn = (zprob * softplus_tf(-lo) + (1.0 - zprob) * softplus_tf(lo)) * \
                cfg.constrains_num_gamma
        zkl = concrete_kl(y, plo, Tq, lo, Tq)
        zkl = torch.where(stop < thr, zkl, torch.zeros_like(zkl))
        stop = stop + (1.0 - zp)
        act = stop < thr
        canvas = canvas + torch.where(act[:, None], zp[:, None] * wr, torch.zeros_like(wr))
        skl = 0.5 * ((((gclv - clv) - 1.0) + cvar / gcvar) + (cm - gcm) ** 2 / gcvar)
        gv = torch.exp(gslv)
        shkl = 0.5 * ((((gslv - slv) - 1.0) + svar / gv) + (sm - gsm) ** 2 / gv).sum(1)
        vkl = 0.5 * ((((vplv - lv) - 1.0) + torch.exp(lv) / cfg.vae_prior_variance) +
                     (mu - cfg.vae_prior_mean) ** 2 / cfg.vae_prior_variance).sum(1)
        lw = 1.0 if live else 0.0
        kl = zkl + torch.where(act, skl + shkl + vkl, torch.zeros_like(skl))
        for k, v in (("scale", s), ("shift", shift), ("zprob", zprob), ("kl", kl * lw),
                     ("prn", prn * lw)):
            rec[k].append(v)
        zprev, ssprev, hg_prev = zl, torch.cat([sl, cl[:, None]], 1), hg
    Tx = steps
    S = {k: torch.stack(v[:Tx], 1) for k, v in rec.items()}
    Cf = float(C)
    sc = S["scale"] * Cf
    amin, amax = cfg.constrains_area_minmax
    area = (torch.clamp(amax - sc, min=0.0) + torch.clamp(sc - amin, min=0.0)).mean(1)
    cx = (S["shift"][..., 0] + 1.0) * Cf / 2.0
    cy = (S["shift"][..., 1] + 1.0) * Cf / 2.0
    outl = (torch.clamp(-(cx - 0.5 * sc), min=0) + torch.clamp(-(cy - 0.5 * sc), min=0) +
            torch.clamp(cx + 0.5 * sc - Cf, min=0) + torch.clamp(cy + 0.5 * sc - Cf, min=0)).sum(1)
    size = torch.clamp((sc[:, :, None] - sc[:, None, :]).abs() - 3.0, min=0).sum((1, 2))
    md = torch.maximum((cx[:, :, None] - cx[:, None, :]).abs(),
                       (cy[:, :, None] - cy[:, None, :]).abs())
    smean = (sc[:, :, None] + sc[:, None, :]) / 2.0
    over = (torch.clamp(smean - md, min=0) * (1.0 - torch.eye(Tx, dtype=dt))).sum((1, 2))
    pr = (S["prn"].sum(1) + cfg.constrains_area_gamma * area + over * cfg.constrains_bbox_gamma +
          outl * cfg.constrains_bbox_gamma + size * cfg.constrains_sharesize_gamma)
    margin, elem = torch.zeros((), dtype=dt), torch.zeros(B, dtype=dt)
    if cfg.constrains_margin_gamma > 1e-8:
        obj = torch.tensor([[1.0 if t < k else 0.0 for t in range(Tx)]
                            for k in cfg.constrains_num], dtype=dt)
        margin = (_sce(obj.mean(0), _logit8(S["zprob"].mean(0))) *
                  cfg.constrains_margin_gamma).sum()
        elem = _sce(obj[None], _logit8(S["zprob"])[:, None, :]).sum(2).min(1).values * \
            cfg.constrains_num_element_gamma
    loss = (S["kl"].sum(1) + pr + elem).mean() + margin + (canvas_cotangent * canvas).sum()
    return {"loss": loss, "T": Tx}


# --------------------------------------------------------- generation -----
def generate(cfg, P, noise, G, learned=True):
    """tests/asr_gen_ref.generate with the scale latent of :1170-1201: the
    gen_scale heads on (hg_t, generated shift latent), cl = gcm + eps_scale
    sqrt(exp(gclv)).  The write scale stays the constant (:1203-1205), so cl
    reaches the output through the next step's LSTM input only."""
    if not learned:
        return gref.generate(cfg, P, noise, G)
    T, C, W = cfg.max_steps, cfg.canvas_size, cfg.windows_size
    H, Z = cfg.rnn_units, cfg.vae_latent_dimensions
    nz = {k: np.ascontiguousarray(v, f32) for k, v in noise.items()}
    thr, temp = f32(cfg.stopping_threshold), f32(cfg.z_pres_temperature)
    lik_std = f32(cfg.vae_likelihood_std)
    s = gref.write_scale(cfg)
    vpm, vplv = f32(cfg.vae_prior_mean), ao.f32log(cfg.vae_prior_variance)
    cg, hg, hg_prev = (np.zeros((G, H), f32) for _ in range(3))
    z_prev, ss_prev = np.zeros((G, Z), f32), np.zeros((G, 3), f32)
    stop, digits = np.zeros(G, f32), np.zeros(G, np.int32)
    canvas = np.zeros((G, C * C), f32)
    st, cls = [], []
    for t in range(T):
        if not np.any(stop < thr):
            break
        hg, cg = _lstm(P, "gen_rnn_running", np.concatenate([z_prev, ss_prev], axis=1), hg, cg, H)
        hm = _relu(ao.dense_chain(hg, _p(P, "gen_shift/dense/kernel"), _p(P, "gen_shift/dense/bias")))
        m = ao.dense_chain(hm, _p(P, "gen_shift/dense_1/kernel"), _p(P, "gen_shift/dense_1/bias"))
        hv = _relu(ao.dense_chain(hg, _p(P, "gen_shift/dense_2/kernel"),
                                  _p(P, "gen_shift/dense_2/bias")))
        lv = ao.dense_chain(hv, _p(P, "gen_shift/dense_3/kernel"), _p(P, "gen_shift/dense_3/bias"))
        sl = m + nz["eps_shift"][t] * np.sqrt(_math(EXP, lv))
        xy = _math(TANH, sl)
        gcm, gclv = scale_heads(P, "gen_scale", hg, sl)
        cl = gcm + nz["eps_scale"][t] * np.sqrt(_math(EXP, gclv))
        ss = np.concatenate([sl, cl[:, None]], axis=1).astype(f32)
        z = (vpm + nz["eps_z"][t] * np.sqrt(_math(EXP, np.array([vplv], f32)))[0]).astype(f32)
        d1 = _math(SOFTPLUS, ao.dense_chain(z, _p(P, "vae/generative_1/weights"),
                                            _p(P, "vae/generative_1/biases")))
        d2 = _math(SOFTPLUS, ao.dense_chain(d1, _p(P, "vae/generative_2/weights"),
                                            _p(P, "vae/generative_2/biases")))
        mean = ao.dense_chain(d2, _p(P, "vae/gen_mean/weights"), _p(P, "vae/gen_mean/biases"))
        window = np.where(_math(SIGMOID, mean + nz["eps_x"][t] * lik_std) > nz["u_x"][t],
                          f32(1), f32(0)).astype(f32)
        theta = np.zeros((G, 6), f32)
        theta[:, 0] = theta[:, 4] = f32(1) / s
        theta[:, 2] = -xy[:, 0] / s
        theta[:, 5] = -xy[:, 1] / s
        recon = ao.stn(window.reshape(G, W, W), theta, (C, C)).reshape(G, C * C)
        if cfg.fix_steps is not None:
            lo = np.full(G, 100.0 if t < cfg.fix_steps else -100.0, f32)
        else:
            hp = _relu(ao.dense_chain(hg_prev, _p(P, "z_pres/prior/dense/kernel"),
                                      _p(P, "z_pres/prior/dense/bias")))
            lo = ao.dense_chain(hp, _p(P, "z_pres/prior/dense_1/kernel"),
                                _p(P, "z_pres/prior/dense_1/bias"))[:, 0]
        u = nz["u"][t]
        y = (lo + (_math(LOG, u + f32(1e-9)) - _math(LOG, (f32(1) - u) + f32(1e-9)))) / temp
        zp = np.rint(_math(SIGMOID, y)).astype(f32)
        stop = stop + (f32(1) - zp)
        act = stop < thr
        digits = digits + act.astype(np.int32)
        canvas = canvas + np.where(act[:, None], zp[:, None] * recon, f32(0)).astype(f32)
        hg_prev, z_prev, ss_prev = hg, z, ss
        st.append(theta)
        cls.append(cl)
    for a in (cg, hg, ss, canvas, stop):
        assert a.dtype == f32
    return {"canvas": canvas, "st_back": np.stack(st), "digits": digits, "T": len(st),
            "scale_latent": np.stack(cls)}


# -------------------------------------------------------------- cases -----
# input sets: k -> (batch, seed); parameters seed, noise seed + 1, images seed + 2
SETS = {1: (6, 30), 2: (12, 20)}
_CASES = {}


def case(k, fix_steps=None, train=True):
    """Config (tests/test_gpu_asr.py::_cfg: T = 4, every regulariser on),
    parameters with the gen_scale block, noise, images, the oracle's
    fixed-prior forward and the numpy restatement for both priors: computed
    once per variant, shared and left unchanged by the tests."""
    key = (k, fix_steps, train)
    if key in _CASES:
        return _CASES[key]
    from test_gpu_asr import _cfg
    batch, seed = SETS[k]
    cfg = _cfg(batch=batch, fix_steps=fix_steps, train=train)
    P = so.init_params(cfg, seed=seed, bias_scale=0.05)
    n_fixed = len(P)
    P.update(gen_scale_params(cfg, seed + 100, bias_scale=0.05))
    nz = so.make_noise(cfg, seed=seed + 1)
    x, tg = ao.synthetic_canvases(cfg.batch, seed=seed + 2)
    ref = so.forward(cfg, P, nz, x, tg)
    c = {"cfg": cfg, "P": P, "P_fixed": dict(list(P.items())[:n_fixed]), "nz": nz, "x": x,
         "tg": tg, "ref": ref,
         "fixed": scale_kl_numpy(cfg, P, nz, x, ref, False),
         "learned": scale_kl_numpy(cfg, P, nz, x, ref, True)}
    for v in list(P.values()) + list(nz.values()) + [x] + \
            [a for d in (ref, c["fixed"], c["learned"]) for a in d.values()
             if isinstance(a, np.ndarray)]:
        v.setflags(write=False)
    _CASES[key] = c
    return c


def check_case(c):
    """The inputs exercise the masks and the learned prior: 4 executed steps,
    active and inactive images at step 1, and a learned-prior KL that differs
    from the fixed-prior one wherever an image is active."""
    assert c["ref"]["T"] == 4
    act = c["learned"]["act"]
    assert act[1].any() and not act[1].all()
    assert act[3].any() and not act[0].all()  # some run all four steps, some stop at step 0
    a, b = c["learned"]["scale_kl"], c["fixed"]["scale_kl"]
    assert np.all(a[act] != b[act])
    assert np.all(a[~act] == 0) and np.all(b[~act] == 0)
