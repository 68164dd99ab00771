"""csrc/summary.hip through ops.summary_histograms / ops.summary_groups against
the NumPy restatement (tests/summary_ref.py).

Histograms: counts, min, max, num and nonfinite are exact; sum and sum_squares
are within n * 2^-52 * sum|x| (resp. sum x^2), the bound of any summation
order of n doubles; two launches give the same bits; counts is pre-filled
with garbage.  Applied mode: denom bit-equal to the restatement on exactly
summable chunk sums, counts exact against the float32 (g * clip) / denom; on
a model, Adam's first moment pins the histogram's values to what Adam
consumed.  Grouped means: within one float32 spacing, counts exact."""
import numpy as np
import pytest
import torch

import summary_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4096
NB = 1551


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _ops():
    from mog_air import ops
    return ops


def _thr():
    from mog_air import summaries
    return torch.from_numpy(summaries.bucket_thresholds()).to(DEV)


class Table:
    """The optimizer's table (params.ParamStore._build_optim_table) of tensors
    of the given lengths, each starting 64-element aligned."""

    def __init__(self, lens, total=None):
        self.lens = list(lens)
        self.offs, off = [], 0
        for n in self.lens:
            self.offs.append(off)
            off += (n + 63) // 64 * 64
        self.total = off if total is None else total
        assert off <= self.total
        bt, bs = [], []
        for i, n in enumerate(self.lens):
            for c0 in range(0, n, CHUNK):
                bt.append(i)
                bs.append(c0)
        self.n_blocks = len(bt)
        self.t_off = torch.tensor(self.offs, dtype=torch.int64, device=DEV)
        self.t_len = torch.tensor(self.lens, dtype=torch.int64, device=DEV)
        self.t_bt = torch.tensor(bt, dtype=torch.int32, device=DEV)
        self.t_bs = torch.tensor(bs, dtype=torch.int64, device=DEV)
        self.bt = bt

    def outputs(self, garbage=True):
        V = len(self.lens)
        counts = torch.full((V, NB), -12345 if garbage else 0, dtype=torch.int32, device=DEV)
        stats = torch.full((V, 6), 777.0, dtype=torch.float64, device=DEV)
        work = torch.full((6 * max(1, self.n_blocks),), float("nan"), dtype=torch.float64,
                          device=DEV)
        return counts, stats, work

    def run(self, buf, **applied):
        counts, stats, work = self.outputs()
        _ops().summary_histograms(buf, self.t_off, self.t_len, self.t_bt, self.t_bs,
                                  self.n_blocks, _thr(), counts, stats, work, **applied)
        return counts.cpu().numpy(), stats.cpu().numpy()

    def slices(self, host):
        return [host[o:o + n] for o, n in zip(self.offs, self.lens)]


def _check_against_ref(values, counts, stats):
    """One tensor: values float32 (what the kernel classified)."""
    want_c, want_s = ref.histogram(values)
    assert np.array_equal(counts.astype(np.int64), want_c)
    assert stats[0] == want_s[0] and stats[1] == want_s[1]      # min, max
    assert stats[2] == want_s[2] and stats[5] == want_s[5]      # num, nonfinite
    assert counts.sum() == want_s[2]
    d = values[np.isfinite(values)].astype(np.float64)
    n = max(d.size, 1)
    bound_s, bound_q = n * 2.0 ** -52 * np.abs(d).sum(), n * 2.0 ** -52 * (d * d).sum()
    print("n", d.size, "sum", stats[3], want_s[3], bound_s, "sq", stats[4], want_s[4], bound_q)
    assert abs(stats[3] - want_s[3]) <= bound_s
    assert abs(stats[4] - want_s[4]) <= bound_q


# ------------------------------------------------------------- raw mode ----
LENS = (1, 3, 255, 4096, 4097, 8193)
FLT_MAX = np.finfo(np.float32).max


def _raw_case():
    table = Table(LENS + (0,), total=2 ** 15)
    rest = table.total - table.offs[-1]
    table = Table(LENS + (rest,), total=2 ** 15)
    assert table.offs[-1] + rest == 2 ** 15
    rng = np.random.default_rng(5)
    host = np.zeros(table.total, np.float32)
    t = table.slices(host)
    t[0][:] = np.float32(-0.0)
    t[1][:] = [np.nan, 1.0, -np.inf]
    t[2][:] = np.nan                                        # an all-NaN tensor
    lim = np.sqrt(6.0 / (64 + 64))
    t[3][:] = rng.uniform(-lim, lim, 4096).astype(np.float32)   # Glorot uniform
    t[4][:] = rng.normal(0.0, 1e-4, 4097).astype(np.float32)
    t[5][:] = np.float32(0.1)                               # 8193 copies of one value
    # around every limit: the float32 below it, float32(limit), the one above, both signs
    pos = ref.positive_limits()
    near = pos.astype(np.float32)
    edge = np.concatenate([np.nextafter(near, np.float32(0)), near,
                           np.nextafter(near, np.float32(np.inf))])
    special = np.float32([0.0, -0.0, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, np.nan, np.inf, -np.inf])
    fill = np.concatenate([edge, -edge, special])
    assert len(fill) == 774 * 6 + 9 and len(fill) < rest
    t[6][:len(fill)] = fill
    t[6][len(fill):] = rng.normal(0.0, 1e-4, rest - len(fill)).astype(np.float32)
    return table, host


def test_hist_raw_against_restatement():
    table, host = _raw_case()
    buf = torch.from_numpy(host).to(DEV)
    counts, stats = table.run(buf)
    for v, values in enumerate(table.slices(host)):
        _check_against_ref(values, counts[v], stats[v])
    # the all-NaN tensor: nothing added
    assert stats[2][2] == 0 and stats[2][5] == 255 and counts[2].sum() == 0
    assert stats[2][0] == ref.DBL_MAX and stats[2][1] == -ref.DBL_MAX
    # 8193 copies of one value: one bucket
    assert (counts[5] > 0).sum() == 1 and counts[5].max() == 8193
    # two launches: the same bits
    counts2, stats2 = table.run(buf)
    assert counts.tobytes() == counts2.tobytes() and stats.tobytes() == stats2.tobytes()


def test_hist_empty_tensor_and_small_tables():
    """A table with a zero-length tensor (no block of its own) and a single
    short tensor: every output row is still written."""
    table = Table((5, 0, 70))
    host = np.arange(table.total, dtype=np.float32) - 3
    counts, stats = table.run(torch.from_numpy(host).to(DEV))
    for v, values in enumerate(table.slices(host)):
        _check_against_ref(values, counts[v], stats[v])
    assert stats[1].tolist() == [ref.DBL_MAX, -ref.DBL_MAX, 0, 0, 0, 0]


# --------------------------------------------------------- applied mode ----
def test_hist_applied_against_restatement():
    clip = 0.75
    table = Table((8193, 4097, 100))
    rng = np.random.default_rng(6)
    host = rng.normal(0.0, 0.3, table.total).astype(np.float32)
    host[table.offs[2]:table.offs[2] + 100] = 0.0
    host[table.offs[2] + 3] = 2.5  # (the chunk sums are crafted, not derived)
    # exactly summable chunk sums: norm 4 > clip, norm 0.5 < clip, norm 0
    chunks = [[4.0, 8.0, 4.0], [0.125, 0.125], [0.0]]
    sumsq = torch.tensor([c for t in chunks for c in t], dtype=torch.float32, device=DEV)
    assert len(sumsq) == table.n_blocks
    denom = torch.full((3,), -1.0, dtype=torch.float32, device=DEV)
    counts, stats = table.run(torch.from_numpy(host).to(DEV), sumsq=sumsq, clip=clip, denom=denom)
    denom = denom.cpu().numpy()
    for v, g in enumerate(table.slices(host)):
        values, want_denom = ref.applied(g, clip, chunks[v])
        assert denom[v].tobytes() == np.float32(want_denom).tobytes()
        _check_against_ref(values, counts[v], stats[v])
    assert denom.tolist() == [4.0, 0.75, 0.75]


def _model():
    from mog_air.air_model import AIRModel
    from oracle import air_oracle as ao
    m = AIRModel(max_steps=3, scale_prior_variance=0.05, z_pres_prior_log_odds=-0.01,
                 learning_rate=1e-4, gradient_clipping_norm=1.0, cnn=False, train=True,
                 scope="summ_test", device=DEV)
    x, k = ao.synthetic_canvases(8, seed=13)
    return m, x, k


def _applied_fetch(m):
    from mog_air import summaries
    p = m.params
    V = len(p.specs)
    counts = torch.full((V, NB), -1, dtype=torch.int32, device=DEV)
    stats = torch.empty((V, 6), dtype=torch.float64, device=DEV)
    work = torch.empty((6 * p.n_blocks,), dtype=torch.float64, device=DEV)
    denom = torch.empty((V,), dtype=torch.float32, device=DEV)
    thr = torch.from_numpy(summaries.bucket_thresholds()).to(DEV)
    _ops().summary_histograms(p.grad, p.t_off, p.t_len, p.t_bt, p.t_bs, p.n_blocks, thr, counts,
                              stats, work, sumsq=p.sumsq, clip=m.gradient_clipping_norm,
                              denom=denom)
    return counts.cpu().numpy(), stats.cpu().numpy(), denom.cpu().numpy()


def _gc(m, denom):
    """Every variable's applied gradient rebuilt on the host from the
    post-step params.grad and the kernel's denom, in float32."""
    g = m.params.grad.cpu().numpy()
    clip = np.float32(m.gradient_clipping_norm)
    out = []
    for v, (name, shape) in enumerate(m.params.specs):
        o, n = m.params.offsets[name], int(np.prod(shape))
        out.append(((g[o:o + n] * clip).astype(np.float32) / denom[v]).astype(np.float32))
    return out


def _moments(m, buf):
    host = getattr(m.params, buf).cpu().numpy()
    return [host[m.params.offsets[n]:m.params.offsets[n] + int(np.prod(s))].copy()
            for n, s in m.params.specs]


def test_hist_applied_is_what_adam_consumed():
    m, x, k = _model()
    one_minus_b1 = np.float32(1.0) - np.float32(0.9)
    m.step(x, k)
    counts, stats, denom = _applied_fetch(m)
    gcs = _gc(m, denom)
    for v, (gc, mom) in enumerate(zip(gcs, _moments(m, "m"))):
        # Adam's first moment from zero: m = gc * (1 - beta1), bit for bit
        want = (gc * one_minus_b1).astype(np.float32)
        assert np.array_equal(mom, want), m.params.specs[v][0]
        _check_against_ref(gc, counts[v], stats[v])
    assert np.all(denom >= np.float32(m.gradient_clipping_norm))
    # the captured step: its first call runs eagerly and captures, the second replays
    m.train_step_graphed(x, k)
    before = _moments(m, "m")
    m.train_step_graphed(x, k)
    counts, stats, denom = _applied_fetch(m)
    gcs = _gc(m, denom)
    for v, (gc, m0, m1) in enumerate(zip(gcs, before, _moments(m, "m"))):
        want = (m0 + ((gc - m0).astype(np.float32) * one_minus_b1).astype(np.float32))
        assert np.array_equal(m1, want.astype(np.float32)), m.params.specs[v][0]
        _check_against_ref(gc, counts[v], stats[v])


# ---------------------------------------------------------------- groups ----
TMAX, MAXD = 6, 6


def _group_inputs(B, t_exec, seed):
    rng = np.random.default_rng(seed)
    target = rng.choice([1, 3], B).astype(np.int32)
    steps = rng.integers(0, t_exec + 1, B).astype(np.int32)
    per = [rng.normal(50, 20, B).astype(np.float32), (rng.random(B) < 0.5).astype(np.float32),
           rng.normal(300, 90, B).astype(np.float32)]
    recs = []
    for q in range(6):
        r = rng.normal(q, 1.0, (TMAX, B)).astype(np.float32)
        r[t_exec:] = np.nan  # whatever the workspace holds there is not read
        recs.append(r)
    live = np.zeros(TMAX + 1, np.int32)
    live[:t_exec] = 1
    return target, steps, per, recs, live


def _run_groups(target, steps, per, recs, live, acc, accumulate=False):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    _ops().summary_groups(d(target), d(steps), *[d(a) for a in per], *[d(r) for r in recs],
                          d(live), MAXD, acc, accumulate=accumulate)


def _check_groups(acc, s, c):
    acc = acc.cpu().numpy()
    assert np.array_equal(acc[..., 1], c)
    got, want = ref.means(acc[..., 0], acc[..., 1]), ref.means(s, c)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok])))
    return got


@pytest.mark.parametrize("B", [1, 5, 67, 1030])
@pytest.mark.parametrize("t_exec", [1, 3, 6])
def test_groups_against_restatement(B, t_exec):
    target, steps, per, recs, live = _group_inputs(B, t_exec, seed=B * 10 + t_exec)
    acc = torch.full((4 + 6 * TMAX, MAXD + 2, 2), float("nan"), dtype=torch.float64, device=DEV)
    _run_groups(target, steps, per, recs, live, acc)
    s, c = ref.groups(target, steps, per, recs, t_exec, MAXD)
    got = _check_groups(acc, s, c)
    # targets are drawn from {1, 3}: the other groups are empty and give NaN
    assert np.all(np.isnan(got[:, [0, 2, 4, 5, 6]])) and not np.any(np.isnan(got[:4, MAXD + 1]))
    first = acc.clone()
    _run_groups(target, steps, per, recs, live, acc)
    assert acc.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()


def test_groups_two_chunks_equal_one_launch():
    B, t_exec = 67, 3
    target, steps, per, recs, live = _group_inputs(B, t_exec, seed=3)
    shape = (4 + 6 * TMAX, MAXD + 2, 2)
    one = torch.empty(shape, dtype=torch.float64, device=DEV)
    _run_groups(target, steps, per, recs, live, one)
    two = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    for n, (lo, hi) in enumerate(((0, 40), (40, B))):
        _run_groups(target[lo:hi], steps[lo:hi], [a[lo:hi] for a in per],
                    [r[:, lo:hi] for r in recs], live, two, accumulate=n > 0)
    a, b = one.cpu().numpy(), two.cpu().numpy()
    assert np.array_equal(a[..., 1], b[..., 1])
    s, c = ref.groups(target, steps, per, recs, t_exec, MAXD)
    _check_groups(two, s, c)
    with np.errstate(invalid="ignore"):
        assert np.allclose(a[..., 0], b[..., 0], rtol=1e-13, atol=0)


def test_groups_against_a_real_infer():
    from mog_air.air_model import AIRModel
    from oracle import air_oracle as ao
    m = AIRModel(max_steps=3, max_digits=3, scale_prior_variance=0.05,
                 z_pres_prior_log_odds=-0.01, cnn=False, train=False, scope="summ_infer",
                 device=DEV)
    x, k = ao.synthetic_canvases(8, seed=13)
    m.infer(x, k)
    ws = m._ws
    T, D = m.max_steps, m.max_digits
    acc = torch.empty((4 + 6 * T, D + 2, 2), dtype=torch.float64, device=DEV)
    tg = torch.as_tensor(k).to(DEV, torch.int32)
    _ops().summary_groups(tg, ws.digits, ws.bce, ws.acc_b, ws.loss_b, ws.scale, ws.zprob, ws.zkl,
                          ws.skl, ws.shkl, ws.vkl, ws.live, D, acc)
    t_exec = m.executed_steps

    def rec(a):  # the model's accessor [B, T_exec] -> [T, B], NaN past T_exec
        out = np.full((T, len(k)), np.nan, np.float32)
        out[:t_exec] = a.cpu().numpy().T
        return out
    recs = [rec(m.rec_scales[:, :, 0]), rec(m.z_pres_probs), rec(m.z_pres_kls),
            rec(m.scale_kls), rec(m.shift_kls), rec(m.vae_kls)]
    per = [m.reconstruction_loss.cpu().numpy(), m.accuracy_instance.cpu().numpy(),
           m.per_image_loss.cpu().numpy()]
    s, c = ref.groups(np.asarray(k), m.rec_num_digits.cpu().numpy(), per, recs, t_exec, D)
    _check_groups(acc, s, c)


# -------------------------------------------------------------- refusals ----
def test_hist_refusals_leave_outputs_untouched():
    ops = _ops()
    table = Table((100, 5000))
    buf = torch.zeros(table.total, device=DEV)
    thr = _thr()
    counts, stats, work = table.outputs()
    denom = torch.full((2,), -1.0, device=DEV)
    sumsq = torch.zeros(table.n_blocks, device=DEV)
    keep = [t.clone() for t in (counts, stats, denom)]

    def call(**kw):
        a = dict(buf=buf, t_off=table.t_off, t_len=table.t_len, t_bt=table.t_bt, t_bs=table.t_bs,
                 n_blocks=table.n_blocks, thresholds=thr, counts=counts, stats=stats, work=work)
        a.update(kw)
        ops.summary_histograms(**a)

    bad = [dict(buf=buf.cpu()), dict(buf=buf.double()), dict(buf=buf.reshape(2, -1)),
           dict(buf=torch.zeros(2 * table.total, device=DEV)[::2]),
           dict(counts=counts.to(torch.int64)), dict(counts=counts[:, :100].contiguous()),
           dict(counts=counts[:1]), dict(stats=stats.float()), dict(stats=stats[:, :5]),
           dict(work=work[:5]), dict(thresholds=thr[:100]), dict(thresholds=thr.double()),
           dict(thresholds=thr.cpu()), dict(n_blocks=table.n_blocks + 1),
           dict(t_bt=table.t_bt.to(torch.int64)), dict(t_off=table.t_off.to(torch.int32)),
           dict(t_len=table.t_len[:1]),
           # applied mode: all three together, sumsq of the table's n_blocks
           dict(sumsq=sumsq), dict(sumsq=sumsq, clip=1.0), dict(clip=1.0, denom=denom),
           dict(sumsq=sumsq[:-1], clip=1.0, denom=denom),
           dict(sumsq=torch.zeros(table.n_blocks + 1, device=DEV), clip=1.0, denom=denom),
           dict(sumsq=sumsq, clip=0.0, denom=denom), dict(sumsq=sumsq, clip=1.0, denom=denom[:1]),
           dict(sumsq=sumsq.cpu(), clip=1.0, denom=denom),
           dict(sumsq=sumsq, clip=1.0, denom=denom.double())]
    for kw in bad:
        with pytest.raises((ValueError, RuntimeError)):
            call(**kw)
    torch.cuda.synchronize()
    for t, k in zip((counts, stats, denom), keep):
        assert torch.equal(t, k)
    call()  # and the good call goes through
    assert int(counts.sum()) == 5100


def test_groups_refusals_leave_outputs_untouched():
    ops = _ops()
    B = 5
    target, steps, per, recs, live = _group_inputs(B, 3, seed=1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    good = dict(target=d(target), steps=d(steps), bce=d(per[0]), acc_b=d(per[1]),
                loss_b=d(per[2]), scale=d(recs[0]), zprob=d(recs[1]), zkl=d(recs[2]),
                skl=d(recs[3]), shkl=d(recs[4]), vkl=d(recs[5]), live=d(live), max_digits=MAXD)
    acc = torch.full((4 + 6 * TMAX, MAXD + 2, 2), -7.0, dtype=torch.float64, device=DEV)
    keep = acc.clone()
    big = torch.zeros((9, B), device=DEV)
    bad = [dict(target=good["target"].cpu()), dict(target=good["target"].long()),
           dict(target=good["target"][:0]), dict(steps=good["steps"][:3]),
           dict(steps=good["steps"].float()), dict(bce=good["bce"].double()),
           dict(loss_b=good["loss_b"][:2]), dict(scale=good["scale"][:, :3].contiguous()),
           dict(zkl=good["zkl"][:4]), dict(vkl=good["vkl"].t()), dict(live=good["live"][:3]),
           dict(live=good["live"].long()), dict(max_digits=9), dict(max_digits=-1),
           dict(max_digits=5),  # acc of another max_digits
           dict(scale=big, zprob=big, zkl=big, skl=big, shkl=big, vkl=big),  # Tmax 9
           dict(skl=good["skl"].cpu())]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        with pytest.raises((ValueError, RuntimeError)):
            ops.summary_groups(acc=acc, **a)
    with pytest.raises((ValueError, RuntimeError)):
        ops.summary_groups(acc=acc.float(), **good)
    with pytest.raises((ValueError, RuntimeError)):
        ops.summary_groups(acc=acc[:10], **good)
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)
    ops.summary_groups(acc=acc, **good)
    assert float(acc[0, MAXD + 1, 1]) == B
