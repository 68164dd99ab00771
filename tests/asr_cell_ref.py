"""TEST HELPER (not collected) -- references and input tables for the AIR-ASR
cell and loss kernels of csrc/asr_cell.hip taken alone
(tests/test_asr_cell_ref.py pins them on the CPU,
tests/test_gpu_asr_cell_kernels.py holds the kernels against them).

* ``terms_ref``: the structural terms and their gradient dreg from the record
  layout the kernels read, through oracle.asr_torch.structural_terms (float64
  torch, TF's tie conventions); ``terms_fwd_f32`` restates the forward in numpy
  float32 in the kernels' operation order.
* ``step_ref``: one loop step (oracle.asr_torch.asr_forward's per-image part)
  from the step kernel's operands, every gradient by autograd on the scalar

      L = <dtheta_fwd, theta_fwd> + <dtheta_back, theta_back>
          + sum_b dot_b (act_b ? z_b : 0) + <dreg, (s, tx, ty, lo)> + <dss, ss>
          + grad_scale sum_b (act_old_b zkl_b + act_b (skl_b + shkl_b))

  (dtheta_back arrives already scaled by act * z, as the kernel documents: it
  is the STN-write backward of the canvas term).  ``step_fwd_f32`` restates the
  forward in numpy float32 in the kernel's order.
* the input builders: deterministic, explicit seeds, the case tables of the
  GPU test.

"Column" below: one output array of a kernel (one record slot, one douts
column, one dpre layer, one of dreg's four components).  ``bound`` is the
suite's "within rounding of float64": max(8 E32, 2^-20 max|ref64|) with E32 the
largest |ref32 - ref64| of the column, ref32 the same reference in float32."""
import dataclasses
import os
import re
from typing import Optional

import numpy as np
import torch

from oracle import air_oracle as ao
from oracle import asr_oracle as so
from oracle import asr_torch as st
from oracle.air_torch import concrete_kl, softplus_tf

from math_spec_cases import (EXP, LOG, LOG1P, SIGMOID, SOFTPLUS, TANH, logistic_noise,
                             oracle_math)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS = 64


def _record_slots():
    """Slot names of rec[step][30][B] from the ABI comment of include/mog_air.h."""
    with open(os.path.join(ROOT, "include", "mog_air.h")) as f:
        txt = f.read()
    m = re.search(r"Record layout rec\[step\]\[(\d+)\]\[B\]:(.*?)\(zkl", txt, re.S)
    names = m.group(2).replace("*", " ").split()
    assert len(names) == int(m.group(1)) == 30, names
    return {n: i for i, n in enumerate(names)}


Q = _record_slots()
NQ = len(Q)
# output-layer weights in the ABI order of w[20] / gw[8] (include/mog_air.h)
(W_IS1, B_IS1, W_IS3, B_IS3, W_IC0, B_IC0, W_IC1, B_IC1, W_IC2, B_IC2, W_IC3, B_IC3,
 W_GS1, B_GS1, W_GS3, B_GS3, W_ZP1, B_ZP1, W_ZL1, B_ZL1) = range(20)
W_GC0, B_GC0, W_GC1, B_GC1, W_GC2, B_GC2, W_GC3, B_GC3 = range(8)
DOUTS = ("sm0", "sm1", "slv0", "slv1", "lo", "gsm0", "gsm1", "gslv0", "gslv1", "plo", "cm",
         "clv", "gcm", "gclv")


def f32r(x) -> float:
    """x as the float the kernels receive."""
    return float(F(x))


def bound(ref64, ref32):
    r64 = np.asarray(ref64, np.float64)
    e32 = float(np.abs(np.asarray(ref32, np.float64) - r64).max()) if r64.size else 0.0
    top = float(np.abs(r64).max()) if r64.size else 0.0
    return max(8.0 * e32, 2.0 ** -20 * top)


# =================================================================== terms ====
def loss_cfg(cons=(1, 3), g_num=0.5, g_margin=100.0, g_element=10.0, g_bbox=1.0, g_size=0.3,
             g_area=0.2, area_minmax=(17.0, 23.0), C=50):
    """An AsrConfig whose gammas are the float32 values the kernels receive."""
    return so.AsrConfig(canvas_size=C, constrains_num=tuple(cons), constrains_num_gamma=f32r(g_num),
                        constrains_margin_gamma=f32r(g_margin),
                        constrains_num_element_gamma=f32r(g_element),
                        constrains_bbox_gamma=f32r(g_bbox),
                        constrains_sharesize_gamma=f32r(g_size), constrains_area_gamma=f32r(g_area),
                        constrains_area_minmax=(f32r(area_minmax[0]), f32r(area_minmax[1])))


def gammas(cfg):
    """gammas[8] in the ABI order: num, margin, element, bbox, size, area, area_min, area_max."""
    return [cfg.constrains_num_gamma, cfg.constrains_margin_gamma,
            cfg.constrains_num_element_gamma, cfg.constrains_bbox_gamma,
            cfg.constrains_sharesize_gamma, cfg.constrains_area_gamma,
            cfg.constrains_area_minmax[0], cfg.constrains_area_minmax[1]]


def executed_steps(live, T):
    return int((np.asarray(live)[:T] != 0).sum())


def terms_ref(rec, vkl, zmask, live, cfg, grad_scale=1.0, inv_batch_global=None,
              dtype=torch.float64):
    """rec [T, 30, B], vkl / zmask [T, B], live [>= T]; steps t >= Tx are never
    read.  Values from the recorded slots (what the kernels read); dreg
    [T, 4, B] = d(grad_scale sum_b (pr_b + element_b) + margin) / d(s, tx, ty,
    lo) with zprob = sigmoid(lo) and prn recomputed from lo as in the model;
    the margin's batch mean is zsum * inv_batch_global (default 1 / B)."""
    rec = np.asarray(rec)
    T, nq, B = rec.shape
    assert nq == NQ
    Tx = executed_steps(live, T)
    inv = 1.0 / B if inv_batch_global is None else float(inv_batch_global)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype)  # noqa: E731
    R = lambda k: t(rec[:Tx, Q[k], :].T.reshape(B, Tx))  # noqa: E731
    kw = dict(zsum_reduce=lambda z: z, global_batch=1.0 / inv)
    with torch.no_grad():
        v = st.structural_terms(cfg, R("s"), torch.stack([R("tx"), R("ty")], 2), R("zprob"),
                                R("prn"), **kw)
        zm = t(np.asarray(zmask)[:Tx].T.reshape(B, Tx))
        vk = t(np.asarray(vkl)[:Tx].T.reshape(B, Tx))
        klsum = (R("zkl").sum(1) + R("skl").sum(1) + R("shkl").sum(1) +
                 torch.where(zm != 0, vk, torch.zeros_like(vk)).sum(1))
        out = {k: v[k].numpy().astype(np.float64) for k in ("area", "out", "size", "overlap", "pr",
                                                            "element")}
        out["margin"] = float(v["margin"])
        out["klsum"] = klsum.numpy().astype(np.float64)
        out["loss"] = out["klsum"] + out["pr"] + out["element"]
        out["zsum"] = R("zprob").sum(0).numpy().astype(np.float64)
    s, tx, ty, lo = (R(k).requires_grad_() for k in ("s", "tx", "ty", "lo"))
    zprob = torch.sigmoid(lo)
    prn = torch.zeros_like(lo)
    if cfg.constrains_num_gamma > 1e-8:
        prn = (zprob * softplus_tf(-lo) + (1.0 - zprob) * softplus_tf(lo)) * cfg.constrains_num_gamma
    g = st.structural_terms(cfg, s, torch.stack([tx, ty], 2), zprob, prn, **kw)
    total = float(grad_scale) * (g["pr"] + g["element"]).sum() + g["margin"]
    dreg = np.zeros((T, 4, B), np.float64)
    if Tx > 0:
        grads = torch.autograd.grad(total, (s, tx, ty, lo), allow_unused=True)
        for k, gr in enumerate(grads):
            if gr is not None:
                dreg[:Tx, k, :] = gr.numpy().T
    out["dreg"] = dreg
    out["Tx"] = Tx
    return out


def _sce32(z, x):
    """sigmoid_ce of csrc/asr_cell.hip: ((x > 0 ? x : 0) - x z) + log1p(exp(-|x|))."""
    ax = np.where(x < 0, -x, x).astype(F)
    return ((np.where(x > 0, x, F(0)).astype(F) - x * z) + oracle_math(LOG1P, oracle_math(EXP, -ax)))


def _logit8_32(p):
    e = F(1e-8)
    return oracle_math(LOG, p + e) - oracle_math(LOG, (F(1) - p) + e)


def terms_fwd_f32(rec, live, cfg):
    """asr_terms_kernel's area / out / size / overlap and asr_finalize_kernel's
    element in numpy float32, one rounding per operation in the kernels' order."""
    rec = np.asarray(rec, F)
    T, _, B = rec.shape
    Tx = executed_steps(live, T)
    C = F(cfg.canvas_size)
    g = [F(v) for v in gammas(cfg)]
    amin, amax = g[6], g[7]
    z = np.zeros(B, F)
    mx0 = lambda a: np.maximum(a, F(0)).astype(F)  # noqa: E731
    sc = [rec[t, Q["s"]] * C for t in range(Tx)]
    cx = [((rec[t, Q["tx"]] + F(1)) * C) / F(2) for t in range(Tx)]
    cy = [((rec[t, Q["ty"]] + F(1)) * C) / F(2) for t in range(Tx)]
    area = z.copy()
    for t in range(Tx):
        area = area + (mx0(amax - sc[t]) + mx0(sc[t] - amin))
    area = area / F(Tx) if Tx > 0 else z.copy()
    outl, size, over = z.copy(), z.copy(), z.copy()
    for i in range(Tx):
        mnx, mny = cx[i] - F(0.5) * sc[i], cy[i] - F(0.5) * sc[i]
        mxx, mxy = cx[i] + F(0.5) * sc[i], cy[i] + F(0.5) * sc[i]
        outl = outl + (((mx0(F(-1) * mnx) + mx0(F(-1) * mny)) + mx0(mxx - C)) + mx0(mxy - C))
        for j in range(Tx):
            size = size + mx0(np.abs(sc[i] - sc[j]) - F(3))
            md = np.maximum(np.abs(cx[i] - cx[j]), np.abs(cy[i] - cy[j]))
            smean = (sc[i] + sc[j]) / F(2)
            over = over + mx0(smean - md) * (F(0) if i == j else F(1))
    elem = z.copy()
    if g[1] > 1e-8:
        best = None
        for k in cfg.constrains_num:
            s = z.copy()
            for t in range(Tx):
                s = s + _sce32(F(1) if t < k else F(0), _logit8_32(rec[t, Q["zprob"]]))
            best = s if best is None else np.minimum(best, s)
        elem = best * g[2]
    res = {"area": area, "out": outl, "size": size, "overlap": over, "element": elem}
    for k, a in res.items():
        assert a.dtype == F, k
    return res


def _sigmoid32(lo):
    return oracle_math(SIGMOID, np.asarray(lo, F))


def _finish_record(rec, g_num, rng):
    """zprob = sigmoid(lo) and prn = entropy(lo) g_num as the step kernel
    records them; the KL slots positive random, the rest N(0, 1)."""
    T, _, B = rec.shape
    lo = rec[:, Q["lo"]]
    p = _sigmoid32(lo).reshape(lo.shape)
    rec[:, Q["zprob"]] = p
    ent = (p * oracle_math(SOFTPLUS, F(-1) * lo).reshape(lo.shape) +
           (F(1) - p) * oracle_math(SOFTPLUS, lo).reshape(lo.shape))
    rec[:, Q["prn"]] = ent * F(g_num) if g_num > 1e-8 else F(0)
    for k in ("zkl", "skl", "shkl"):
        rec[:, Q[k]] = rng.uniform(0, 3, (T, B)).astype(F)
    return rec


def _live(T, Tx):
    live = np.zeros(T + 1, np.int32)
    live[:Tx] = 1
    return live


def terms_random(B, T, Tx, seed, g_num=0.5):
    """Random records [T, 30, B]; records and vkl / zmask of steps >= Tx are NaN."""
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((T, NQ, B)).astype(F)
    rec[:, Q["s"]] = rng.uniform(0.05, 0.95, (T, B)).astype(F)
    rec[:, Q["tx"]] = rng.uniform(-0.95, 0.95, (T, B)).astype(F)
    rec[:, Q["ty"]] = rng.uniform(-0.95, 0.95, (T, B)).astype(F)
    rec[:, Q["lo"]] = (rng.standard_normal((T, B)) * 3).astype(F)
    _finish_record(rec, g_num, rng)
    vkl = rng.uniform(0, 40, (T, B)).astype(F)
    zmask = (rng.random((T, B)) < 0.6).astype(F)
    rec[Tx:], vkl[Tx:], zmask[Tx:] = np.nan, np.nan, np.nan
    return {"rec": rec, "vkl": vkl, "zmask": zmask, "live": _live(T, Tx), "B": B, "T": T, "Tx": Tx}


# ---- the branch table: one image per row, T = 3 executed steps ----
BRANCH_AREA = (12.5, 25.0)  # sc = 50 k / 64 reaches both bounds exactly (k = 16, 32)


def size_pair_exactly_3():
    """Two float32 scales whose canvas sizes differ by exactly 3 in float32
    (25 n / 2^k is never 3: no dyadic pair exists at C = 50) and by more than 3
    in float64, so the hinge |d| - 3 >= 0 is on in both; found by a fixed
    search over neighbours of 0.42 and 0.36."""
    a0, b0 = F(0.42), F(0.36)
    for i in range(64):
        a = a0
        for _ in range(i):
            a = np.nextafter(a, F(1))
        for j in range(64):
            b = b0
            for _ in range(j):
                b = np.nextafter(b, F(0))
            if F(a * F(50)) - F(b * F(50)) == F(3) and np.float64(a) * 50 - np.float64(b) * 50 > 3:
                return a, b
    raise AssertionError("no pair")


def _geometry_rows():
    """(s, tx, ty) x 3 steps per row; k / 64 values unless said (sc = 50 s and
    the centres 25 (t + 1) are then exact in float32)."""
    k = lambda *v: tuple(x / 64.0 for x in v)  # noqa: E731
    sa, sb = (float(v) for v in size_pair_exactly_3())
    far_x, far_y = k(-56 + 8, 0, 56 - 8), k(0, 0, 0)  # three small boxes in a row never meet
    rows = [
        # area (bounds 12.5 / 25): below, inside, above; on min, on max, inside
        (k(8, 24, 48), k(-32, 0, 32), k(-32, 32, 0)),
        (k(16, 32, 24), k(-32, 28, 0), k(-32, 0, 36)),
        # out of canvas, each side alone (step 0), sc = 12.5
        (k(16, 16, 16), k(-56, 0, 40), k(0, -40, 40)),
        (k(16, 16, 16), k(56, 0, -40), k(0, -40, 40)),
        (k(16, 16, 16), k(0, -40, 40), k(-56, 0, 40)),
        (k(16, 16, 16), k(0, -40, 40), k(56, 0, -40)),
        # exactly touching: left / right / top, then bottom
        (k(16, 16, 16), k(-48, 48, 0), k(0, 0, -48)),
        (k(16, 16, 16), k(0, -40, 40), k(48, 0, -40)),
        # share-size: |d| below 3; above 3 with both signs; two equal of three; exactly 3
        (k(8, 11, 9), far_x, far_y),
        (k(12, 20, 4), far_x, far_y),
        (k(10, 10, 26), far_x, far_y),
        ((sa, sb, sa), k(-40, 40, 0), k(-40, 40, 40)),
        # overlap (boxes 0 and 1; box 2 small in a corner): x dominant, y dominant,
        # tied, coincident centres, disjoint, smean == md exactly
        (k(24, 24, 8), k(0, 16, 56), k(0, 8, 56)),
        (k(24, 24, 8), k(0, -8, 56), k(0, 16, 56)),
        (k(24, 24, 8), k(0, 16, 56), k(0, -16, 56)),
        (k(24, 24, 8), k(0, 0, 56), k(0, 0, 56)),
        (k(8, 8, 8), k(-40, 0, 40), k(-40, 0, 40)),
        (k(16, 16, 8), k(-16, 16, 56), k(0, 8, -56)),
        # all three coincide (every pair: sign 0, size tie)
        (k(20, 20, 20), k(4, 4, 4), k(-4, -4, -4)),
    ]
    return rows


P_TINY, P_HALF, P_ONE = 1e-7, 0.5, 1 - 2.0 ** -24
_LOGIT = lambda p: float(np.log(p) - np.log1p(-p))  # noqa: E731
# lo per step: the zprob specials, the exact two-way tie of cons (1, 2) (step 1 at
# 0.5), both later steps at 0.5 (ties cons (1, 3) too), and random rows
LO_ROWS = ((_LOGIT(P_TINY), 0.0, _LOGIT(P_ONE)), (1.25, 0.0, -0.75), (-2.0, 0.0, 0.0),
           (_LOGIT(P_ONE), _LOGIT(P_TINY), 0.0), None, None, None)
BRANCH_CONS = ((1,), (1, 3), (1, 2), (0, 1, 2, 3, 4, 5, 6, 7))


def terms_branch_table(seed=5):
    """Every geometry row under every lo row: B = 19 * 7 images, T = Tx = 3."""
    rng = np.random.default_rng(seed)
    geo = _geometry_rows()
    T, B = 3, len(geo) * len(LO_ROWS)
    rec = rng.standard_normal((T, NQ, B)).astype(F)
    for b in range(B):
        s, tx, ty = geo[b % len(geo)]
        lo = LO_ROWS[b % len(LO_ROWS)]
        if lo is None:
            lo = rng.standard_normal(3) * 3
        for t in range(T):
            rec[t, Q["s"], b], rec[t, Q["tx"], b], rec[t, Q["ty"], b] = s[t], tx[t], ty[t]
            rec[t, Q["lo"], b] = lo[t]
    assert np.gcd(len(geo), len(LO_ROWS)) == 1
    _finish_record(rec, 0.5, rng)
    vkl = rng.uniform(0, 40, (T, B)).astype(F)
    zmask = (rng.random((T, B)) < 0.6).astype(F)
    return {"rec": rec, "vkl": vkl, "zmask": zmask, "live": _live(T, T), "B": B, "T": T, "Tx": T}


# ==================================================================== step ====
@dataclasses.dataclass
class StepCfg:
    step: int = 0
    train: bool = True
    fix_steps: int = -1
    thr: float = 0.9
    temperature: float = 0.1
    gcm: float = -1.0
    gcvar: float = 0.05
    g_num: float = 0.5
    live: int = 1  # live[step]

    @property
    def gclv32(self) -> float:
        return float(ao.f32log(self.gcvar))


def _step_graph(inp, cfg: StepCfg, learned, dt):
    """The forward of one step in torch; returns (values, leaves, kept)."""
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dt)  # noqa: E731
    W = [t(a) for a in inp["w"]]
    GW = [t(a) for a in inp["gw"]] if learned else None
    pre = [None if a is None else t(a).requires_grad_() for a in inp["pre"]]
    raw = [t(a).requires_grad_() for a in inp["raw"][:4 if learned else 2]]
    eps_shift, eps_scale, u = t(inp["eps_shift"]), t(inp["eps_scale"]), t(inp["u"])
    stop_old = t(inp["stop_old"])
    B = stop_old.shape[0]
    Tq = f32r(cfg.temperature)
    thr = f32r(cfg.thr)
    kept = {}

    def keep(name, v):
        if v.requires_grad:
            v.retain_grad()
        kept[name] = v
        return v

    h = [None if p is None else torch.relu(p) for p in pre]
    sm = keep("sm", h[0] @ W[W_IS1] + W[B_IS1])
    slv = keep("slv", h[1] @ W[W_IS3] + W[B_IS3])
    gsm = keep("gsm", h[3] @ W[W_GS1] + W[B_GS1])
    gslv = keep("gslv", h[4] @ W[W_GS3] + W[B_GS3])
    lo = keep("lo", (h[2] @ W[W_ZL1] + W[B_ZL1])[:, 0])
    if cfg.fix_steps >= 0:
        plo = torch.full((B,), 100.0 if cfg.step < cfg.fix_steps else -100.0, dtype=dt)
    else:
        plo = (h[5] @ W[W_ZP1] + W[B_ZP1])[:, 0]
    plo = keep("plo", plo)
    svar = torch.exp(slv)
    sl = sm + eps_shift * torch.sqrt(svar)
    shift = torch.tanh(sl)

    def pair(rm, rv, Ws, o):
        fin, outs = [], []
        for r, (w0, b0, w1, b1) in ((rm, Ws[o:o + 4]), (rv, Ws[o + 4:o + 8])):
            hid = torch.relu(r + sl @ w0[256:258] + b0)
            fin.append(hid)
            outs.append((torch.cat([hid, sl], 1) @ w1 + b1)[:, 0])
        return fin, outs

    fin67, (cm, clv) = pair(raw[0], raw[1], W, W_IC0)
    cm, clv = keep("cm", cm), keep("clv", clv)
    cvar = torch.exp(clv)
    cl = cm + eps_scale * torch.sqrt(cvar)
    s = torch.sigmoid(cl)
    fin = list(fin67)
    if learned:
        fin89, (gcm, gclv) = pair(raw[2], raw[3], GW, W_GC0)
        gcm, gclv = keep("gcm", gcm), keep("gclv", gclv)
        gcvar = torch.exp(gclv)
        fin += fin89
    else:
        gcm, gcvar = f32r(cfg.gcm), f32r(cfg.gcvar)
        gclv = cfg.gclv32 if dt == torch.float32 else float(np.log(gcvar))
    tx, ty = shift[:, 0], shift[:, 1]
    zr = torch.zeros_like(s)
    theta_fwd = torch.stack([s, zr, tx, zr, s, ty], 1)
    theta_back = torch.stack([1.0 / s, zr, -tx / s, zr, 1.0 / s, -ty / s], 1)
    ss = torch.cat([sl, cl[:, None]], 1)
    y = (lo + (torch.log(u + 1e-9) - torch.log(1.0 - u + 1e-9))) / Tq
    z = torch.sigmoid(y)
    if not cfg.train:
        z = torch.round(z).detach()
    zprob = torch.sigmoid(lo)
    g_num = f32r(cfg.g_num)
    if g_num > 1e-8:
        prn = (zprob * softplus_tf(-lo) + (1.0 - zprob) * softplus_tf(lo)) * g_num
    else:
        prn = torch.zeros_like(lo)
    zkl = concrete_kl(y, plo, Tq, lo, Tq)
    act_old = stop_old < thr
    stop = stop_old + (1.0 - z)
    act = stop < thr
    skl = 0.5 * ((((gclv - clv) - 1.0) + cvar / gcvar) + (cm - gcm) ** 2 / gcvar)
    gv = torch.exp(gslv)
    shkl = 0.5 * ((((gslv - slv) - 1.0) + svar / gv) + (sm - gsm) ** 2 / gv).sum(1)
    zero = torch.zeros_like(s)
    one = torch.ones_like(s)
    fl = lambda m: torch.where(m, one, zero)  # noqa: E731
    live = one * float(cfg.live != 0)
    slots = {"sm0": sm[:, 0], "sm1": sm[:, 1], "slv0": slv[:, 0], "slv1": slv[:, 1],
             "sl0": sl[:, 0], "sl1": sl[:, 1], "cm": cm, "clv": clv, "cl": cl, "s": s, "tx": tx,
             "ty": ty, "gsm0": gsm[:, 0], "gsm1": gsm[:, 1], "gslv0": gslv[:, 0],
             "gslv1": gslv[:, 1], "plo": plo, "lo": lo, "y": y, "z": z, "act_old": fl(act_old),
             "act": fl(act), "live": live, "zkl": torch.where(act_old, zkl, zero),
             "skl": torch.where(act, skl, zero), "shkl": torch.where(act, shkl, zero),
             "prn": prn * live, "zprob": zprob}
    if learned:
        slots["gcm"], slots["gclv"] = gcm, gclv
    vals = {"slots": slots, "theta_fwd": theta_fwd, "theta_back": theta_back, "ss": ss, "scale": s,
            "shift": shift, "zprob": zprob, "zmask": fl(act), "zval": z,
            "zc": torch.where(act, z, zero), "stop": stop, "act": act, "fin": fin}
    return vals, (pre, raw), kept


def _step_values(vals, inp, learned):
    n = lambda v: v.detach().numpy()  # noqa: E731
    nq = NQ if learned else Q["gcm"]
    rec = np.stack([n(vals["slots"][k]) for k in sorted(vals["slots"], key=Q.get)])
    assert rec.shape[0] == nq
    out = {k: n(vals[k]) for k in ("theta_fwd", "theta_back", "ss", "scale", "shift", "zprob",
                                   "zmask", "zval", "zc", "stop")}
    out["rec"] = rec
    act = n(vals["act"])
    out["digits"] = np.asarray(inp["digits"], np.int32) + act.astype(np.int32)
    out["live_next"] = bool(act.any())
    out["fin"] = [n(v) for v in vals["fin"]]
    return out


def step_loss(vals, cot, dtype=torch.float64):
    """The module docstring's L, per image [B] (L is their sum)."""
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype)  # noqa: E731
    sl = vals["slots"]
    zero = torch.zeros_like(sl["s"])
    dreg = t(cot["dreg"])
    L = (t(cot["dtheta_fwd"]) * vals["theta_fwd"]).sum(1) + \
        (t(cot["dtheta_back"]) * vals["theta_back"]).sum(1) + \
        t(cot["dot"]) * torch.where(vals["act"], vals["zval"], zero) + \
        (dreg[0] * sl["s"] + dreg[1] * sl["tx"] + dreg[2] * sl["ty"] + dreg[3] * sl["lo"])
    if cot.get("dss") is not None:
        L = L + (t(cot["dss"]) * vals["ss"]).sum(1)
    # (the record's KL slots are the masked values: act_old zkl, act skl, act shkl)
    return L + f32r(cot["grad_scale"]) * (sl["zkl"] + sl["skl"] + sl["shkl"])


def step_ref(inp, cfg: StepCfg, learned, cot=None, dtype=torch.float64):
    """One loop step.  Returns (forward values, gradients or None): with
    cotangents ``cot`` (dtheta_fwd, dtheta_back [B, 6], dot [B], dreg [4, B],
    dss [B, 3] or None, grad_scale), douts [B, 12 | 14] and dpre[k] [B, 64]
    (None where the layer is absent) by autograd on the module docstring's L."""
    vals, (pre, raw), kept = _step_graph(inp, cfg, learned, dtype)
    fwd = _step_values(vals, inp, learned)
    if cot is None:
        return fwd, None
    step_loss(vals, cot, dtype).sum().backward()
    g = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy()  # noqa: E731
    cols = [g(kept["sm"])[:, 0], g(kept["sm"])[:, 1], g(kept["slv"])[:, 0], g(kept["slv"])[:, 1],
            g(kept["lo"]), g(kept["gsm"])[:, 0], g(kept["gsm"])[:, 1], g(kept["gslv"])[:, 0],
            g(kept["gslv"])[:, 1], g(kept["plo"]), g(kept["cm"]), g(kept["clv"])]
    if learned:
        cols += [g(kept["gcm"]), g(kept["gclv"])]
    dpre = [None if p is None else g(p) for p in pre] + [g(r) for r in raw]
    return fwd, {"douts": np.stack(cols, 1), "dpre": dpre}


def _scale_pair32(rm, rv, sl, Ws, o):
    """hidden = relu(fma(sl1, w[257], fma(sl0, w[256], raw)) + b); out = the
    66-term chain over concat([hidden, sl]) + b (csrc/asr_cell.hip phases 3, 4)."""
    fin, outs = [], []
    eye = np.eye(HS, dtype=F)
    for r, (w0, b0, w1, b1) in ((rm, Ws[o:o + 4]), (rv, Ws[o + 4:o + 8])):
        # one k-ordered chain per unit: raw * 1 (exact), 0-weighted others, then the two
        # latent terms
        a = ao.dense_chain(np.concatenate([r, sl], 1), np.concatenate([eye, w0[256:258]], 0))
        a = a + b0[None, :]
        hid = np.where(a > 0, a, F(0)).astype(F)
        fin.append(hid)
        outs.append(ao.dense_chain(np.concatenate([hid, sl], 1), w1, b1)[:, 0])
    return fin, outs


def step_fwd_f32(inp, cfg: StepCfg, learned):
    """asr_step_fwd_kernel in numpy float32, one rounding per operation in the
    kernel's order: ao.dense_chain fma chains, mog_math.h transcendentals
    (oracle_math), the oracle's concrete_kl."""
    W = [np.ascontiguousarray(a, F) for a in inp["w"]]
    hid = [None if a is None else np.maximum(np.asarray(a, F), F(0)) for a in inp["pre"]]
    es, e_s, u = (np.asarray(inp[k], F) for k in ("eps_shift", "eps_scale", "u"))
    stop_old = np.asarray(inp["stop_old"], F)
    B = stop_old.shape[0]
    Tq, thr = F(cfg.temperature), F(cfg.thr)
    sm = ao.dense_chain(hid[0], W[W_IS1], W[B_IS1])
    slv = ao.dense_chain(hid[1], W[W_IS3], W[B_IS3])
    gsm = ao.dense_chain(hid[3], W[W_GS1], W[B_GS1])
    gslv = ao.dense_chain(hid[4], W[W_GS3], W[B_GS3])
    lo = ao.dense_chain(hid[2], W[W_ZL1], W[B_ZL1])[:, 0]
    if cfg.fix_steps >= 0:
        plo = np.full(B, 100.0 if cfg.step < cfg.fix_steps else -100.0, F)
    else:
        plo = ao.dense_chain(hid[5], W[W_ZP1], W[B_ZP1])[:, 0]
    svar = oracle_math(EXP, slv)
    sl = sm + es * np.sqrt(svar)
    fin, (cm, clv) = _scale_pair32(inp["raw"][0], inp["raw"][1], sl, W, W_IC0)
    gcm = np.full(B, cfg.gcm, F)
    gcvar = np.full(B, cfg.gcvar, F)
    gclv = np.full(B, cfg.gclv32, F)
    if learned:
        GW = [np.ascontiguousarray(a, F) for a in inp["gw"]]
        fin89, (gcm, gclv) = _scale_pair32(inp["raw"][2], inp["raw"][3], sl, GW, W_GC0)
        gcvar = oracle_math(EXP, gclv)
        fin = fin + fin89
    shift = oracle_math(TANH, sl)
    tx, ty = shift[:, 0], shift[:, 1]
    cvar = oracle_math(EXP, clv)
    cl = cm + e_s * np.sqrt(cvar)
    s = oracle_math(SIGMOID, cl)
    zr = np.zeros(B, F)
    theta_fwd = np.stack([s, zr, tx, zr, s, ty], 1)
    theta_back = np.stack([F(1) / s, zr, -tx / s, zr, F(1) / s, -ty / s], 1)
    y = (lo + logistic_noise(u)) / Tq
    z = oracle_math(SIGMOID, y)
    if not cfg.train:
        z = np.rint(z).astype(F)
    zprob = oracle_math(SIGMOID, lo)
    prn = np.zeros(B, F)
    if F(cfg.g_num) > 1e-8:
        ent = zprob * oracle_math(SOFTPLUS, F(-1) * lo) + (F(1) - zprob) * oracle_math(SOFTPLUS, lo)
        prn = ent * F(cfg.g_num)
    zkl = np.array([ao.concrete_kl(float(y[b]), float(plo[b]), float(Tq), float(lo[b]), float(Tq))
                    for b in range(B)], F)
    act_old = stop_old < thr
    stop = stop_old + (F(1) - z)
    act = stop < thr
    dc = cm - gcm
    skl = F(0.5) * ((((gclv - clv) - F(1)) + cvar / gcvar) + (dc * dc) / gcvar)
    shs = np.zeros(B, F)
    for d in range(2):
        gv = oracle_math(EXP, gslv[:, d])
        sv = oracle_math(EXP, slv[:, d])
        dd = sm[:, d] - gsm[:, d]
        shs = shs + ((((gslv[:, d] - slv[:, d]) - F(1)) + sv / gv) + (dd * dd) / gv)
    live = cfg.live != 0
    one = np.ones(B, F)
    slots = {"sm0": sm[:, 0], "sm1": sm[:, 1], "slv0": slv[:, 0], "slv1": slv[:, 1],
             "sl0": sl[:, 0], "sl1": sl[:, 1], "cm": cm, "clv": clv, "cl": cl, "s": s, "tx": tx,
             "ty": ty, "gsm0": gsm[:, 0], "gsm1": gsm[:, 1], "gslv0": gslv[:, 0],
             "gslv1": gslv[:, 1], "plo": plo, "lo": lo, "y": y, "z": z,
             "act_old": np.where(act_old, one, zr), "act": np.where(act, one, zr),
             "live": one * F(live), "zkl": np.where(act_old, zkl, zr), "skl": np.where(act, skl, zr),
             "shkl": np.where(act, F(0.5) * shs, zr), "prn": prn if live else zr, "zprob": zprob}
    if learned:
        slots["gcm"], slots["gclv"] = gcm, gclv
    rec = np.stack([slots[k] for k in sorted(slots, key=Q.get)]).astype(F)
    out = {"rec": rec, "theta_fwd": theta_fwd, "theta_back": theta_back,
           "ss": np.concatenate([sl, cl[:, None]], 1), "scale": s, "shift": shift, "zprob": zprob,
           "zmask": np.where(act, one, zr), "zval": z, "zc": np.where(act, z, zr), "stop": stop,
           "digits": np.asarray(inp["digits"], np.int32) + act.astype(np.int32),
           "live_next": bool(act.any()), "fin": fin}
    for k, a in out.items():
        if isinstance(a, np.ndarray) and k != "digits":
            assert a.dtype == F, k
    return out


# ---- the per-image case table of the step kernels ----
# (stop_old, u, lo target or None, plo target or None): with thr = 0.9 the
# stopping sum gives (act_old, act) = (1, 1) from 0 with z near 1, (1, 0) "stops
# here" from 0.5 or with z near 0, (0, 0) from 1.25
U_SPECIAL = (0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0)
STEP_ROWS = (
    (0.0, None, 4.0, None), (0.0, None, -4.0, None), (1.25, None, 2.0, None),
    (0.5, 0.5, -1.0, 3.0), (0.0, 0.0, 3.0, -3.0), (0.0, 2.0 ** -24, 100.0, 100.0),
    (0.5, 1 - 2.0 ** -24, -100.0, 100.0), (0.0, 1.0, -100.0, -100.0), (1.25, 0.5, 100.0, -100.0),
    (0.0, None, None, None), (0.5, None, None, None), (0.25, 0.5, 0.25, None),
    (0.0, None, 30.0, -30.0), (0.0, 1.0, 1.5, None),
)
RELU_EDGE_UNITS = (0, 1, 2)  # units of layers 6..9 whose pre-activation is 0, below 0, above 0


def _aim(rng, w, bias, target):
    """A pre-activation row whose relu, through column w, lands on target:
    units whose weight pulls the wrong way are negative (exact zeros after the
    relu), the others scaled."""
    r = np.abs(rng.standard_normal(HS)) + 0.1
    good = np.sign(w) == np.sign(target - bias)
    row = np.where(good, r, -r)
    got = float((np.maximum(row, 0) * w).sum())
    return (row * np.where(good, (target - bias) / got, 1.0)).astype(F)


def step_weights(seed, learned):
    rng = np.random.default_rng(seed)
    n = lambda *s: (rng.standard_normal(s) * 0.25).astype(F)  # noqa: E731
    w = [None] * 20
    for k in (W_IS1, W_IS3, W_GS1, W_GS3):
        w[k], w[k + 1] = n(HS, 2), n(2)
    # the second log-variance column small, so that aiming the first keeps both in [-20, 5]
    for k in (W_IS3, W_GS3):
        w[k][:, 1] *= F(0.2)
        w[k + 1][:] = (F(-1.5), F(-2.5))
    for k in (W_IC0, W_IC2):
        w[k], w[k + 1] = n(258, HS), n(HS)
        w[k][256:258] *= F(0.125)  # (the shift latent reaches +-30 where slv is 5)
    for k in (W_IC1, W_IC3):
        w[k], w[k + 1] = n(HS + 2, 1), n(1)
    for k in (W_ZP1, W_ZL1):
        w[k], w[k + 1] = n(HS, 1), n(1)
    gw = None
    if learned:
        gw = [n(258, HS), n(HS), n(HS + 2, 1), n(1), n(258, HS), n(HS), n(HS + 2, 1), n(1)]
        for k in (W_GC0, W_GC2):
            gw[k][256:258] *= F(0.125)
    for ws in (w, gw):  # (and the output chains' two latent terms likewise)
        if ws is not None:
            for k in ((W_IC1, W_IC3) if ws is w else (W_GC1, W_GC3)):
                ws[k][HS:] *= F(0.125)
    # the relu-edge units of layers 6..9 do not see the shift latent and have the bias
    # 0.5: their pre-activation is raw + 0.5 exactly, in float32 and float64
    for ws, ks in ((w, (W_IC0, W_IC2)), (gw, (W_GC0, W_GC2))):
        if ws is not None:
            for k in ks:
                for q in RELU_EDGE_UNITS:
                    ws[k][256:258, q] = 0
                    ws[k + 1][q] = 0.5
    return w, gw


def step_case(B, offset, seed, cfg: StepCfg, learned):
    """Inputs of one launch: image b is row (offset + b) of STEP_ROWS (cyclic).
    Log-variances are aimed into [-20, 5] on some images; the builder asserts
    that every forward value is finite and that no comparison (stopping
    threshold, relu of layers 6..9) sits within float32 rounding of its edge,
    but for the edges built on purpose."""
    rng = np.random.default_rng(seed)
    w, gw = step_weights(seed + 1, learned)
    nlayers = 4 if learned else 2
    pre = [rng.standard_normal((B, HS)).astype(F) for _ in range(6)]
    raw = [rng.standard_normal((B, HS)).astype(F) for _ in range(nlayers)]
    u = rng.uniform(0.1, 0.9, B).astype(F)
    stop_old = np.zeros(B, F)
    lv_targets = (-20.0, 5.0, -6.0, None, 1.0)
    for b in range(B):
        i = (offset + b) % len(STEP_ROWS)
        so_, uu, lo_t, plo_t = STEP_ROWS[i]
        stop_old[b] = so_
        if uu is not None:
            u[b] = uu
        if lo_t is not None:
            pre[2][b] = _aim(rng, w[W_ZL1][:, 0], w[B_ZL1][0], lo_t)
        if plo_t is not None:
            pre[5][b] = _aim(rng, w[W_ZP1][:, 0], w[B_ZP1][0], plo_t)
        lt = lv_targets[i % len(lv_targets)]
        if lt is not None:  # slv0, gslv0 through the hidden rows; clv (gclv) through raw
            pre[1][b] = _aim(rng, w[W_IS3][:, 0], w[B_IS3][0], lt)
            pre[4][b] = _aim(rng, w[W_GS3][:, 0], w[B_GS3][0], -lt / 4 - 1)
            raw[1][b] = _aim(rng, w[W_IC3][:HS, 0], w[B_IC3][0], lt) - w[B_IC2]
            if learned:
                raw[3][b] = _aim(rng, gw[W_GC3][:HS, 0], gw[B_GC3][0], -lt / 4 - 1) - gw[B_GC2]
        # exact zeros among the hidden pre-activations (the > 0 mask at equality)
        for k in range(6):
            pre[k][b, (7 * b + k) % HS] = 0.0
    for r in raw:  # pre-activation exactly 0, one float32 step below 0.5's negative, above
        edge = np.array([-0.5, np.nextafter(F(-0.5), F(-1)), np.nextafter(F(-0.5), F(0))], F)
        for b in range(B):
            r[b, list(RELU_EDGE_UNITS)] = np.roll(edge, b)
    inp = {"w": w, "gw": gw, "pre": pre, "raw": raw,
           "eps_shift": rng.standard_normal((B, 2)).astype(F),
           "eps_scale": rng.standard_normal(B).astype(F), "u": u, "stop_old": stop_old,
           "digits": rng.integers(0, 5, B).astype(np.int32)}
    if cfg.fix_steps >= 0:
        inp["pre"] = pre[:5] + [None]
    # where a log-variance is large, a smaller noise: the latents stay within 2 (shift) and
    # 3 (scale) of their means (s = sigmoid(-30) would put 1 / s^2 = 1e26 into one image's
    # gradients and hide every other image of the column under the bound)
    for key, m, lv, lim in (("eps_shift", ("sm0", "sm1"), ("slv0", "slv1"), 2.0),
                            ("eps_scale", ("cm",), ("clv",), 3.0)):
        rec = step_ref(inp, cfg, learned)[0]["rec"]
        sd = np.exp(0.5 * np.stack([rec[Q[k]] for k in lv], 1))
        dev = np.abs(inp[key].reshape(B, -1) * sd)
        inp[key] = (inp[key].reshape(B, -1) * np.minimum(1.0, lim / np.maximum(dev, 1e-30))
                    ).astype(F).reshape(inp[key].shape)
    # nudge layer 6..9 pre-activations that happen to sit within 1e-3 of the relu edge
    vals, _, _ = _step_graph(inp, cfg, learned, torch.float64)
    sl = torch.stack([vals["slots"]["sl0"], vals["slots"]["sl1"]], 1).detach().numpy()
    for k, r in enumerate(raw):
        ws = w if k < 2 else gw
        o = (W_IC0, W_IC2, W_GC0, W_GC2)[k]
        a = r.astype(np.float64) + sl @ ws[o][256:258].astype(np.float64) + ws[o + 1]
        near = np.abs(a) < 1e-3
        near[:, list(RELU_EDGE_UNITS)] = False
        r[near] += F(0.01)
    fwd, _ = step_ref(inp, cfg, learned)
    for k in ("rec", "theta_back", "stop"):
        assert np.isfinite(fwd[k]).all(), k
    for k in ("slv0", "slv1", "clv") + (("gclv",) if learned else ()):
        v = fwd["rec"][Q[k]]
        assert (v > -25).all() and (v < 8).all(), (k, v)
    v = fwd["rec"][[Q["gslv0"], Q["gslv1"]]]  # (a prior variance: the KLs divide by it)
    assert (np.abs(v) < 8).all(), v
    thr = f32r(cfg.thr)
    assert (np.abs(fwd["stop"] - thr) > 1e-3).all() and (np.abs(stop_old - thr) > 1e-3).all()
    if not cfg.train:  # z = round(sigmoid(y)): away from the half
        assert (np.abs(torch.sigmoid(torch.tensor(fwd["rec"][Q["y"]])).numpy() - 0.5) > 1e-3).all()
    return inp


def step_cotangents(B, seed, only: Optional[str] = None, dss=True, grad_scale=1.0 / 64):
    """Random cotangents; ``only``: that one alone non-zero (the others exact
    zeros; "grad_scale": all arrays zero)."""
    rng = np.random.default_rng(seed)
    c = {"dtheta_fwd": rng.standard_normal((B, 6)).astype(F),
         "dtheta_back": rng.standard_normal((B, 6)).astype(F),
         "dot": (rng.standard_normal(B) * 3).astype(F),
         "dreg": rng.standard_normal((4, B)).astype(F),
         "dss": rng.standard_normal((B, 3)).astype(F) if dss else None,
         "grad_scale": grad_scale}
    if only is not None:
        for k in ("dtheta_fwd", "dtheta_back", "dot", "dreg", "dss"):
            if k != only and c[k] is not None:
                c[k] = np.zeros_like(c[k])
        if only != "grad_scale":
            c["grad_scale"] = 0.0
        if only == "dss":
            assert dss
    return c


COTANGENTS = ("dtheta_fwd", "dtheta_back", "dot", "dreg", "dss", "grad_scale", None)
