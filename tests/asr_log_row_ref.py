"""The AIR-ASR log row (ops.asr_log_row, csrc/log_row.hip) restated in NumPy
float64 from plain arrays, with the crafted inputs and the two error bars the
tests of the kernel, of ``log_row_`` and of the --graph 1 trainers share.

Definition.  With T_exec = sum(live[:T]):

  z_pres_kl, scale_kl, shift_kl, pr_num
            = (1/B) sum_b sum_{t < T_exec} arec[t, slot, b]   slots zkl, skl, shkl, prn
  vae_kl    = (1/B) sum_b sum_{t < T_exec} fp32(vkl[t, b] * zmask[t, b])
  recon, mse, area_loss, out_loss, size_loss, over_loss, num_min_KL
            = batch means of bce, mse, area, outl, size, over, element
  elbo      = batch mean of fp32(klsum[b] + bce[b])
  num_margin, TotLoss, accu = margin[0], means[0], means[1] (copied)

Bar (a), the kernel against this file: each output within one fp32 spacing of
the float64 value (two float64 summation orders differ by at most
n 2^-53 sum|x|, which can move the fp32 rounding by one step and no more).
Bar (b), a float64 row against an fp32 reduction of the same numbers (the
model's ``log_variables``): |d| <= (n + 2) 2^-24 sum|x| / B, the forward error
of an fp32 sum of n numbers in any order plus the division and one rounding.
"""
import numpy as np

NAMES = ("z_pres_kl", "scale_kl", "shift_kl", "vae_kl", "pr_num", "recon", "mse", "area_loss",
         "out_loss", "size_loss", "over_loss", "num_margin", "num_min_KL", "TotLoss", "elbo",
         "accu")
COPIED = ("num_margin", "TotLoss", "accu")
NQ = 30
SLOTS = {"z_pres_kl": 23, "scale_kl": 24, "shift_kl": 25, "pr_num": 26}  # zkl, skl, shkl, prn
PER_IMAGE = {"recon": "bce", "mse": "mse", "area_loss": "area", "out_loss": "outl",
             "size_loss": "size", "over_loss": "over", "num_min_KL": "element"}
ARRAYS = ("arec", "vkl", "zmask", "live", "bce", "mse", "area", "outl", "size", "over",
          "element", "klsum", "margin", "means")


def _terms(a):
    """name -> the float64 numbers the entry sums (None for a copied entry)."""
    T = a["arec"].shape[0]
    tx = int(np.asarray(a["live"])[:T].sum())
    out = {}
    for name, q in SLOTS.items():
        out[name] = np.asarray(a["arec"], np.float32)[:tx, q].astype(np.float64)
    prod = np.asarray(a["vkl"], np.float32)[:tx] * np.asarray(a["zmask"], np.float32)[:tx]
    out["vae_kl"] = prod.astype(np.float32).astype(np.float64)
    for name, src in PER_IMAGE.items():
        out[name] = np.asarray(a[src], np.float32).astype(np.float64)
    s = np.asarray(a["klsum"], np.float32) + np.asarray(a["bce"], np.float32)
    out["elbo"] = s.astype(np.float32).astype(np.float64)
    return out


def log_row(a):
    """The 16 values in float64 (copied entries: the fp32 value widened)."""
    B = a["arec"].shape[2]
    terms = _terms(a)
    copied = {"num_margin": a["margin"][0], "TotLoss": a["means"][0], "accu": a["means"][1]}
    row = np.empty(len(NAMES), np.float64)
    for i, name in enumerate(NAMES):
        row[i] = float(np.float32(copied[name])) if name in copied else \
            float(np.sum(terms[name], dtype=np.float64)) / B
    return row


def bar_b(a):
    """Bar (b) per entry (0 for the copied ones)."""
    B = a["arec"].shape[2]
    terms = _terms(a)
    bar = np.zeros(len(NAMES), np.float64)
    for i, name in enumerate(NAMES):
        if name not in COPIED:
            x = terms[name]
            bar[i] = (x.size + 2) * 2.0 ** -24 * float(np.abs(x).sum()) / B
    return bar


def crafted(T, t_exec, B, seed):
    """Arrays of mixed sign and magnitude (|x| over six decades); every arec,
    vkl and zmask row at t >= t_exec is NaN; live carries the T + 1 flags of
    the models' workspace."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        v = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)
        return v.astype(np.float32)
    a = {"arec": draw(T, NQ, B), "vkl": draw(T, B), "zmask": draw(T, B)}
    for k in ("arec", "vkl", "zmask"):
        a[k][t_exec:] = np.nan
    live = np.zeros(T + 1, np.int32)
    live[:t_exec] = 1
    a["live"] = live
    for k in ("bce", "mse", "area", "outl", "size", "over", "element", "klsum"):
        a[k] = draw(B)
    a["margin"] = draw(1)
    a["means"] = draw(4)
    return a
