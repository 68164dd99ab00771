"""TEST HELPER (not collected) -- the AIR-ASR generation loop
(air/air_number_bbox_location.py:1124-1361, air/vae.py:51-86) restated in numpy
float32 from primitives the CPU oracle already exports: ``ao.dense_chain``
(one k-ordered fma chain + bias), ``ao.stn``, ``oracle_math_vec`` (the
mog_math.h transcendentals) and the ASR parameter table.

The oracle is compiled with contraction off, so numpy's one rounding per
operation -- every product and sum written as its own float32 operation --
gives the bits C would."""
import ctypes

import numpy as np

from oracle import air_oracle as ao
from oracle import asr_oracle as so

f32 = np.float32
P_ROOT = so.P_ROOT
EXP, LOG, TANH, SIGMOID, SOFTPLUS = 0, 1, 3, 4, 5


def _math(fn, x):
    x = np.ascontiguousarray(x, f32)
    y = np.empty_like(x)
    ao._load().oracle_math_vec(ctypes.c_int(fn), x.ctypes.data_as(ao._FP),
                               y.ctypes.data_as(ao._FP), ctypes.c_int(x.size))
    return y


def _relu(x):
    return np.where(x > 0, x, f32(0)).astype(f32)


def write_scale(cfg):
    """float32(mean(constrains_area_minmax) / canvas_size): the quotient in
    double precision, cast once (:1203-1205)."""
    return f32(float(np.mean(cfg.constrains_area_minmax)) / cfg.canvas_size)


def generate(cfg, P, noise, G):
    """Returns canvas [G, C2], st_back [T_exec, G, 6], digits [G] int32, and
    per executed step the binarised windows [T_exec, G, W2], z_pres [T_exec,
    G], act [T_exec, G] and the written window recon [T_exec, G, C2].
    ``noise``: eps_shift [T,G,2], eps_scale [T,G], eps_z [T,G,Z], eps_x
    [T,G,W2], u_x [T,G,W2], u [T,G]."""
    T, C, W = cfg.max_steps, cfg.canvas_size, cfg.windows_size
    H, Z = cfg.rnn_units, cfg.vae_latent_dimensions
    p = lambda n: np.ascontiguousarray(P[P_ROOT + n], f32)  # noqa: E731
    nz = {k: np.ascontiguousarray(v, f32) for k, v in noise.items()}
    thr, temp = f32(cfg.stopping_threshold), f32(cfg.z_pres_temperature)
    lik_std = f32(cfg.vae_likelihood_std)
    s = write_scale(cfg)
    assert s > 0
    spm, spv = f32(cfg.scale_prior_mean), f32(cfg.scale_prior_variance)
    vpm, vplv = f32(cfg.vae_prior_mean), ao.f32log(cfg.vae_prior_variance)
    cg, hg, hg_prev = (np.zeros((G, H), f32) for _ in range(3))
    z_prev, ss_prev = np.zeros((G, Z), f32), np.zeros((G, 3), f32)
    stop, digits = np.zeros(G, f32), np.zeros(G, np.int32)
    canvas = np.zeros((G, C * C), f32)
    st, wins, zps, acts, recons = [], [], [], [], []
    for t in range(T):
        if not np.any(stop < thr):
            break
        # generative LSTMCell on concat([z_prev, ss_prev, hg]), forget bias +1
        gates = ao.dense_chain(np.concatenate([z_prev, ss_prev, hg], axis=1),
                               p("gen_rnn_running/kernel"), p("gen_rnn_running/bias"))
        gi, gj, gf, go = (gates[:, k * H:(k + 1) * H] for k in range(4))
        cg = cg * _math(SIGMOID, gf + f32(1)) + _math(SIGMOID, gi) * _math(TANH, gj)
        hg = _math(TANH, cg) * _math(SIGMOID, go)
        # gen_shift heads on the new output
        hm = _relu(ao.dense_chain(hg, p("gen_shift/dense/kernel"), p("gen_shift/dense/bias")))
        m = ao.dense_chain(hm, p("gen_shift/dense_1/kernel"), p("gen_shift/dense_1/bias"))
        hv = _relu(ao.dense_chain(hg, p("gen_shift/dense_2/kernel"), p("gen_shift/dense_2/bias")))
        lv = ao.dense_chain(hv, p("gen_shift/dense_3/kernel"), p("gen_shift/dense_3/bias"))
        shift_latent = m + nz["eps_shift"][t] * np.sqrt(_math(EXP, lv))
        xy = _math(TANH, shift_latent)
        scale_latent = spm + nz["eps_scale"][t] * np.sqrt(spv)
        ss = np.concatenate([shift_latent, scale_latent[:, None]], axis=1).astype(f32)
        # latent and decoder, binarised
        z = vpm + nz["eps_z"][t] * np.sqrt(_math(EXP, np.array([vplv], f32)))[0]
        d1 = _math(SOFTPLUS, ao.dense_chain(z, p("vae/generative_1/weights"),
                                            p("vae/generative_1/biases")))
        d2 = _math(SOFTPLUS, ao.dense_chain(d1, p("vae/generative_2/weights"),
                                            p("vae/generative_2/biases")))
        mean = ao.dense_chain(d2, p("vae/gen_mean/weights"), p("vae/gen_mean/biases"))
        samples = _math(SIGMOID, mean + nz["eps_x"][t] * lik_std)
        window = np.where(samples > nz["u_x"][t], f32(1), f32(0)).astype(f32)
        # backward transform with the constant scale
        theta = np.zeros((G, 6), f32)
        theta[:, 0] = theta[:, 4] = f32(1) / s
        theta[:, 2] = -xy[:, 0] / s
        theta[:, 5] = -xy[:, 1] / s
        recon = ao.stn(window.reshape(G, W, W), theta, (C, C)).reshape(G, C * C)
        # z_pres prior log-odds and the rounded concrete sample
        if cfg.fix_steps is not None:
            lo = np.full(G, 100.0 if t < cfg.fix_steps else -100.0, f32)
        else:
            hp = _relu(ao.dense_chain(hg_prev, p("z_pres/prior/dense/kernel"),
                                      p("z_pres/prior/dense/bias")))
            lo = ao.dense_chain(hp, p("z_pres/prior/dense_1/kernel"),
                                p("z_pres/prior/dense_1/bias"))[:, 0]
        u = nz["u"][t]
        logistic = _math(LOG, u + f32(1e-9)) - _math(LOG, (f32(1) - u) + f32(1e-9))
        y = (lo + logistic) / temp
        zp = np.rint(_math(SIGMOID, y)).astype(f32)
        stop = stop + (f32(1) - zp)
        act = stop < thr
        digits = digits + act.astype(np.int32)
        canvas = canvas + np.where(act[:, None], zp[:, None] * recon, f32(0)).astype(f32)
        hg_prev, z_prev, ss_prev = hg, z.astype(f32), ss
        st.append(theta)
        wins.append(window)
        zps.append(zp)
        acts.append(act)
        recons.append(recon)
    for a in (cg, hg, ss, z, canvas, stop):
        assert a.dtype == f32  # no silent promotion anywhere above
    return {"canvas": canvas, "st_back": np.stack(st), "digits": digits, "T": len(st),
            "windows": np.stack(wins), "z_pres": np.stack(zps), "act": np.stack(acts),
            "recon": np.stack(recons)}
