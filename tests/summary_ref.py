"""NumPy restatement of the device summaries (csrc/summary.hip,
mog_air/summaries.py), independent of both: TensorFlow's default histogram
buckets, the float64 moments, the compression of empty runs, the grouped means
of the numeric summaries with the reference's masks and padding
(air/air_model.py:216-264), and the applied gradient value in float32."""
import sys

import numpy as np

DBL_MAX = sys.float_info.max
FLT_MAX = float(np.finfo(np.float32).max)


def positive_limits():
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.asarray(pos, np.float64)


def limits():
    pos = positive_limits()
    return np.concatenate([[-DBL_MAX], -pos[::-1], [0.0], pos, [DBL_MAX]])


def histogram(x):
    """(counts [1551] int64, stats (min, max, num, sum, sum_squares,
    nonfinite)) of a float32 array; NaN / Inf are counted, not added."""
    lim = limits()
    x = np.asarray(x, np.float32).reshape(-1)
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    idx = np.searchsorted(lim, d, side="right")
    counts = np.bincount(idx, minlength=len(lim)).astype(np.int64)
    assert len(counts) == len(lim)
    stats = (d.min() if d.size else DBL_MAX, d.max() if d.size else -DBL_MAX, float(d.size),
             float(np.sum(d)), float(np.sum(d * d)), float((~fin).sum()))
    return counts, stats


def compress(counts):
    """TF's HistogramProto encoding: (bucket_limit, bucket) lists."""
    lim = limits()
    out_l, out_b = [], []
    i = 0
    n = len(counts)
    while i < n:
        end, c = lim[i], counts[i]
        i += 1
        if c <= 0:
            while i < n and counts[i] <= 0:
                end, c = lim[i], counts[i]
                i += 1
            c = 0
        out_l.append(float(end))
        out_b.append(float(c))
    return out_l, out_b


def applied(g, clip, sumsq_chunks):
    """(values, denom) of one tensor as clip_adam consumes them: float32
    throughout.  ``sumsq_chunks`` must be exactly summable (the order of the
    float32 sum then does not matter)."""
    l2 = np.float32(0)
    for s in np.asarray(sumsq_chunks, np.float32):
        l2 = np.float32(l2 + s)
    norm = np.sqrt(l2, dtype=np.float32) if l2 > 0 else l2
    denom = np.float32(max(norm, np.float32(clip)))
    g = np.asarray(g, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((g * np.float32(clip)).astype(np.float32) / denom).astype(np.float32), denom


QUANT = ("steps", "rec_loss", "digit_acc", "total_loss")
STEPQ = ("scale", "z_pres_prob", "z_pres_kl", "scale_kl", "shift_kl", "vae_kl")


def reference_tags(max_steps, max_digits):
    """The tags the reference's naming rule generates, in its order
    (_summarize_by_digit_count / _summarize_by_step, air_model.py:216-264,
    902-920)."""
    tags = []

    def by_count(name):
        for i in range(max_digits + 1):
            tags.append(name + "_" + str(i) + "_dig")
        tags.append(name + "_all_dig")

    for q in QUANT:
        by_count(q)
    for q in STEPQ:
        for i in range(max_steps):
            by_count(q + "_" + str(i + 1) + "_step")
    return tags


def groups(target, steps, per_image, recs, t_exec, max_digits):
    """sum, count [4 + 6 Tmax, max_digits + 2] in float64.  per_image: (bce,
    acc_b, loss_b) [B]; recs: the six [Tmax, B] records in STEPQ order; rows at
    or beyond t_exec are the reference's zero padding (never read)."""
    target, steps = np.asarray(target), np.asarray(steps)
    Tmax = recs[0].shape[0]
    rows = []  # (values [B] float64, mask [B])
    every = np.ones(len(target), bool)
    rows.append((steps.astype(np.float32).astype(np.float64), every))
    for a in per_image:
        rows.append((np.asarray(a, np.float32).astype(np.float64), every))
    for q, rec in enumerate(recs):
        for i in range(Tmax):
            v = (np.asarray(rec[i], np.float32).astype(np.float64) if i < t_exec
                 else np.zeros(len(target)))
            if q == 1:
                m = every
            elif q == 2:
                m = steps > i - 1
            else:
                m = steps > i
            rows.append((v, m))
    s = np.zeros((len(rows), max_digits + 2))
    c = np.zeros_like(s)
    for r, (v, m) in enumerate(rows):
        for g in range(max_digits + 2):
            sel = m & (target == g) if g <= max_digits else m
            s[r, g] = np.sum(v[sel])
            c[r, g] = sel.sum()
    return s, c


def means(s, c):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / c).astype(np.float32)
