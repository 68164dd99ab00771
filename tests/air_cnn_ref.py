"""TEST HELPER (not collected) -- the AIR model's cnn=True image encoder
(air/air_model.py:763-810: conv 5x5 same + relu, max-pool 2x2, twice, then a
third conv, flattened NHWC into the LSTM input) restated from primitives the
CPU oracle exports.

* ``encoder_numpy``: im2col in (ky, kx, cin) order + ``ao.dense_chain`` (one
  fp32 fma chain per output from +0, then + bias) + relu + first-maximum
  pooling -- the arithmetic the HIP forward must reproduce bit for bit.
* ``encoder_torch``: conv2d / max_pool2d (float64-capable), for autograd.
* ``air_cnn_forward_torch``: the loop of oracle/air_torch.py:air_forward with
  the LSTM's x-projection reading the features; ``features=`` replaces the
  encoder (with ``features=images`` it is air_forward itself).
* ``case`` / ``check_case``: inputs and the proof that they are not degenerate.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import air_oracle as ao
from oracle.air_torch import concrete_kl, softplus_tf, transformer

f32 = np.float32
FILTERS = 8
SIDE = 50
NFEAT = 144 * FILTERS
CNN = "air/cnn/"
LAYERS = ("conv1", "conv2", "conv3")
KERNEL = "air/rnn/rnn/basic_lstm_cell/kernel"


def cnn_specs(F=FILTERS):
    out = []
    for layer, cin in zip(LAYERS, (1, F, F)):
        out += [(CNN + layer + "/kernel", (5, 5, cin, F)), (CNN + layer + "/bias", (F,))]
    return out


def cnn_names(F=FILTERS):
    return [n for n, _ in cnn_specs(F)]


def cnn_params(seed, F=FILTERS, bias=0.1):
    """Glorot-uniform HWIO kernels (fan_in 25 Cin, fan_out 25 Cout), biases
    uniform in +-bias (nonzero, so that pooling ties sit at relu(bias) > 0 on
    the flat background and the tie convention shows in the gradients)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in cnn_specs(F):
        if len(shape) == 4:
            lim = np.sqrt(6.0 / (25 * (shape[2] + shape[3])))
            out[name] = rng.uniform(-lim, lim, size=shape).astype(f32)
        else:
            out[name] = rng.uniform(-bias, bias, size=shape).astype(f32)
    return out


# ------------------------------------------------------------- numpy -----
def im2col(a):
    """a [B, H, W, Cin] -> [B H W, 25 Cin], columns in (ky, kx, cin) order,
    `same` padding as two zero pixels on each side."""
    B, H, W, Cin = a.shape
    p = np.zeros((B, H + 4, W + 4, Cin), f32)
    p[:, 2:-2, 2:-2] = a
    cols = [p[:, ky:ky + H, kx:kx + W, :] for ky in range(5) for kx in range(5)]
    return np.ascontiguousarray(np.concatenate(cols, axis=-1).reshape(B * H * W, 25 * Cin))


def conv_numpy(a, w, b):
    B, H, W, _ = a.shape
    out = ao.dense_chain(im2col(a), np.ascontiguousarray(w.reshape(-1, w.shape[-1])), b)
    return np.where(out > 0, out, f32(0)).astype(f32).reshape(B, H, W, w.shape[-1])


def pool_first_max(a):
    """2x2 / stride 2 / valid max-pool of a [B, H, W, C]: values and the index
    (dy 2 + dx) of the FIRST maximum in row-major window order (strict >)."""
    H2, W2 = a.shape[1] // 2, a.shape[2] // 2
    win = [a[:, dy:2 * H2:2, dx:2 * W2:2] for dy in (0, 1) for dx in (0, 1)]
    best, arg = win[0].copy(), np.zeros(win[0].shape, np.int32)
    for j in (1, 2, 3):
        m = win[j] > best
        best = np.where(m, win[j], best)
        arg = np.where(m, j, arg)
    return best, arg


def nonzero_ties(a):
    """Windows of pool_first_max(a) whose maximum is nonzero and attained
    more than once."""
    H2, W2 = a.shape[1] // 2, a.shape[2] // 2
    win = np.stack([a[:, dy:2 * H2:2, dx:2 * W2:2] for dy in (0, 1) for dx in (0, 1)])
    best = win.max(0)
    return int((((win == best).sum(0) > 1) & (best != 0)).sum())


def encoder_planes(x, P):
    """conv1, pool1, conv2, pool2, conv3 of x [B, 2500] (NHWC float32)."""
    x = np.asarray(x, f32).reshape(-1, SIDE, SIDE, 1)
    g = lambda n: np.asarray(P[CNN + n], f32)  # noqa: E731
    c1 = conv_numpy(x, g("conv1/kernel"), g("conv1/bias"))
    p1, _ = pool_first_max(c1)
    c2 = conv_numpy(p1, g("conv2/kernel"), g("conv2/bias"))
    p2, _ = pool_first_max(c2)
    c3 = conv_numpy(p2, g("conv3/kernel"), g("conv3/bias"))
    return c1, p1, c2, p2, c3


def encoder_numpy(x, P):
    """The features [B, 144 F] (index (y 12 + x) F + f) in float32."""
    c3 = encoder_planes(x, P)[-1]
    return c3.reshape(c3.shape[0], -1)


# ------------------------------------------------------------- torch -----
def encoder_torch(x, P, dtype=torch.float64):
    """The features by conv2d / max_pool2d; x [B, 2500] and P's tensors may be
    numpy arrays or torch tensors (autograd flows into torch ones)."""
    t = lambda v: v.to(dtype) if isinstance(v, torch.Tensor) else torch.tensor(  # noqa: E731
        np.asarray(v), dtype=dtype)
    a = t(x).reshape(-1, 1, SIDE, SIDE)
    for i, layer in enumerate(LAYERS):
        w = t(P[CNN + layer + "/kernel"]).permute(3, 2, 0, 1)  # HWIO -> OIHW
        a = torch.relu(Fn.conv2d(a, w, t(P[CNN + layer + "/bias"]), padding=2))
        if i < 2:
            a = Fn.max_pool2d(a, 2)
    return a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)


def _dense(x, P, name, act=None):
    y = x @ P[name + "/weights"] + P[name + "/biases"]
    return act(y) if act is not None else y


def air_cnn_forward_torch(cfg, P, noise, images, targets=None, z_pres_prior_log_odds=None,
                          canvas_cotangent=None, fixed_steps=False, features=None):
    """oracle/air_torch.py:air_forward with the LSTM reading ``features``
    (default: encoder_torch of the images) through the kernel's first
    features.shape[1] rows; the image still feeds the STN read and the loss.
    Also returns ``stop`` [T, B], the stopping sums after each step."""
    dt = images.dtype
    B, T, H = cfg.batch, cfg.max_steps, cfg.rnn_units
    C, W = cfg.canvas_size, cfg.windows_size
    thr = cfg.stopping_threshold
    Tz = cfg.z_pres_temperature
    prior_lo = cfg.z_pres_prior_log_odds if z_pres_prior_log_odds is None else z_pres_prior_log_odds
    mo = ao.marginal_objective(cfg.num_prior, T) if cfg.num_prior is not None else None
    p = "air/rnn/"
    K = P[p + "rnn/basic_lstm_cell/kernel"]
    bK = P[p + "rnn/basic_lstm_cell/bias"]
    feat = encoder_torch(images, P, dt) if features is None else features
    NX = feat.shape[1]
    assert K.shape[0] == NX + H
    h = torch.zeros(B, H, dtype=dt)
    c = torch.zeros(B, H, dtype=dt)
    stop = torch.zeros(B, dtype=dt)
    runloss = torch.zeros(B, dtype=dt)
    digits = torch.zeros(B, dtype=torch.int32)
    canvas = torch.zeros(B, C * C, dtype=dt)
    stops = []
    relu = torch.relu
    slv_p = float(ao.f32log(cfg.scale_prior_variance))
    hlv_p = float(ao.f32log(cfg.shift_prior_variance))
    vlv_p = float(ao.f32log(cfg.vae_prior_variance))
    xk = feat @ K[:NX]
    step = 0
    while step < T:
        live_any = bool((stop < thr).any())
        if not fixed_steps and not live_any:
            break
        live = 1.0 if live_any else 0.0
        g = xk + h @ K[NX:] + bK
        i_, j_, f_, o_ = g.split(H, dim=1)
        c = c * torch.sigmoid(f_ + 1.0) + torch.sigmoid(i_) * torch.tanh(j_)
        h = torch.tanh(c) * torch.sigmoid(o_)
        sm = _dense(_dense(h, P, p + "scale/mean/hidden", relu), P, p + "scale/mean/output")
        sv = _dense(_dense(h, P, p + "scale/log_variance/hidden", relu), P,
                    p + "scale/log_variance/output")
        hm = _dense(_dense(h, P, p + "shift/mean/hidden", relu), P, p + "shift/mean/output")
        hv = _dense(_dense(h, P, p + "shift/log_variance/hidden", relu), P,
                    p + "shift/log_variance/output")
        svar, hvar = torch.exp(sv), torch.exp(hv)
        scale = torch.sigmoid(sm + noise["eps_scale"][step].view(B, 1) * torch.sqrt(svar))
        shift = torch.tanh(hm + noise["eps_shift"][step] * torch.sqrt(hvar))
        s, tx, ty = scale[:, 0], shift[:, 0], shift[:, 1]
        zero = torch.zeros_like(s)
        theta = torch.stack([s, zero, tx, zero, s, ty], 1)
        window = transformer(images.view(B, C, C), theta, (W, W)).reshape(B, W * W)
        v = p + "vae/"
        a1 = _dense(window, P, v + "recognition_1", softplus_tf)
        a2 = _dense(a1, P, v + "recognition_2", softplus_tf)
        mu = _dense(a2, P, v + "rec_mean")
        lv = _dense(a2, P, v + "rec_log_variance")
        z = mu + noise["eps_z"][step] * torch.sqrt(torch.exp(lv))
        d1 = _dense(z, P, v + "generative_1", softplus_tf)
        d2 = _dense(d1, P, v + "generative_2", softplus_tf)
        m = _dense(d2, P, v + "gen_mean")
        r = torch.sigmoid(m + noise["eps_x"][step] * cfg.vae_likelihood_std)
        theta_r = torch.stack([1.0 / s, zero, -tx / s, zero, 1.0 / s, -ty / s], 1)
        wr = transformer(r.view(B, W, W), theta_r, (C, C)).reshape(B, C * C)
        lo = _dense(_dense(h, P, p + "z_pres/log_odds/hidden", relu), P,
                    p + "z_pres/log_odds/output")[:, 0]
        u = noise["u"][step]
        y = (lo + (torch.log(u + 1e-9) - torch.log(1.0 - u + 1e-9))) / Tz
        zp = torch.sigmoid(y)
        if not cfg.train:
            zp = torch.round(zp)
        bias = float(mo[step]) if mo is not None else 0.0
        zkl = concrete_kl(y, prior_lo + bias, Tz, lo, Tz)
        zkl_end = (concrete_kl(y, -100.0, Tz, lo, Tz) if mo is not None
                   else torch.zeros_like(zkl))
        runloss = runloss + live * torch.where(stop < thr, zkl, zkl_end)
        stop = stop + (1.0 - zp)
        stops.append(stop)
        active = stop < thr
        digits = digits + active.to(torch.int32)
        canvas = canvas + torch.where(active.view(B, 1), zp.view(B, 1) * wr,
                                      torch.zeros_like(wr))
        skl = 0.5 * ((slv_p - sv - 1.0 + svar / cfg.scale_prior_variance +
                      (sm - cfg.scale_prior_mean) ** 2 / cfg.scale_prior_variance).sum(1))
        hkl = 0.5 * ((hlv_p - hv - 1.0 + hvar / cfg.shift_prior_variance +
                      (hm - cfg.shift_prior_mean) ** 2 / cfg.shift_prior_variance).sum(1))
        vkl = 0.5 * ((vlv_p - lv - 1.0 + torch.exp(lv) / cfg.vae_prior_variance +
                      (mu - cfg.vae_prior_mean) ** 2 / cfg.vae_prior_variance).sum(1))
        zero_b = torch.zeros_like(skl)
        runloss = runloss + torch.where(active, skl, zero_b)
        runloss = runloss + torch.where(active, hkl, zero_b)
        runloss = runloss + torch.where(active, vkl, zero_b)
        step += 1
    out = {"T": step, "digits": digits, "canvas": canvas, "running_loss": runloss,
           "stop": torch.stack(stops, 0), "features": feat}
    rec = torch.clamp(canvas, 0.0, 1.0)
    if canvas_cotangent is None:
        x = images
        bce = -(x * torch.log(rec + 1e-10) + (1.0 - x) * torch.log(1.0 - rec + 1e-10)).sum(1)
        out["bce"] = bce
        out["loss_b"] = runloss + bce
        out["loss"] = out["loss_b"].mean()
    else:
        out["loss"] = runloss.mean() + (canvas_cotangent * canvas).sum()
    if targets is not None:
        out["accuracy"] = (targets.to(torch.int32) == digits).to(dt).mean()
    return out


# -------------------------------------------------------------- cases ----
_CASES = {}


def corner_canvas():
    """One canvas with content in all four corners and on rows / columns
    24..25 and 48..49 (the pooling seams and the dropped row / column)."""
    rng = np.random.default_rng(77)
    a = np.zeros((SIDE, SIDE), f32)
    for ys in (slice(0, 4), slice(46, 50)):
        for xs in (slice(0, 4), slice(46, 50)):
            a[ys, xs] = rng.uniform(0.1, 1.0, (4, 4))
    for lo in (24, 48):
        a[lo:lo + 2, :] = rng.uniform(0.1, 1.0, (2, SIDE))
        a[:, lo:lo + 2] = rng.uniform(0.1, 1.0, (SIDE, 2))
    return a.reshape(-1)


def case(seed, B, T=3):
    """Inputs of one test case (cached, never modified): synthetic canvases,
    the oracle's parameters with small biases, the LSTM kernel redrawn at the
    features' width, the encoder's six tensors (biases in +-0.1), noise."""
    key = (seed, B, T)
    if key in _CASES:
        return _CASES[key]
    cfg = ao.AirConfig(batch=B, max_steps=T, scale_prior_variance=0.05,
                       z_pres_prior_log_odds=-0.01)
    x, k = ao.synthetic_canvases(B, seed=seed)
    P0 = ao.init_params(cfg, seed=seed + 1000, bias_scale=0.05)  # the cnn=False parameters
    P = dict(P0)
    H = cfg.rnn_units
    lim = np.sqrt(6.0 / (NFEAT + H + 4 * H))
    P[KERNEL] = np.random.default_rng(seed + 2000).uniform(
        -lim, lim, size=(NFEAT + H, 4 * H)).astype(f32)
    P.update(cnn_params(seed + 3000))
    c = dict(cfg=cfg, x=x, k=k, P=P, P0=P0, nz=ao.make_noise(cfg, seed=seed + 4000))
    _CASES[key] = c
    return c


def reference64(c, **kw):
    """The float64 restated loop on a case (no autograd)."""
    with torch.no_grad():
        return air_cnn_forward_torch(
            c["cfg"], {n: torch.tensor(v, dtype=torch.float64) for n, v in c["P"].items()},
            {n: torch.tensor(v, dtype=torch.float64) for n, v in c["nz"].items()},
            torch.tensor(c["x"], dtype=torch.float64), torch.tensor(c["k"]), **kw)


def check_case(c):
    """The inputs are not degenerate: features neither all zero nor all
    positive, pooling ties with a nonzero maximum present, no stopping sum
    within 1e-3 of the threshold in float64, at least two executed steps."""
    c1, p1, c2, p2, c3 = encoder_planes(c["x"], c["P"])
    share = float((c3 != 0).mean())
    assert 0.2 <= share <= 0.95, share
    ties = nonzero_ties(c1) + nonzero_ties(c2[:, :24, :24])
    assert ties >= 100, ties
    ref = reference64(c, fixed_steps=True)
    margin = float((ref["stop"] - c["cfg"].stopping_threshold).abs().min())
    assert margin >= 1e-3, margin
    assert reference64(c)["T"] >= 2
    return share, ties, margin
