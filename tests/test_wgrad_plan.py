"""The weight-gradient planner (mog_air/wgrads.py plan_wgrads) on shapes
alone: which form every call site's gradients take at the row counts and
switches where the forms change.  The expectations are the rules of the code
before the planner, worked out by hand."""
from mog_air.wgrads import (GROUP, SPLITK_BF16, SPLITK_F32, TALL_BF16, TALL_X3, X3_TN,
                            WeightGradients, WgradLaunch, plan_wgrads)

VAE_X3_TN = (0, 1, 5, 6)  # the four 16-byte-row layers (WeightGradients._vae_weight_grads)


def _consts(**switches):
    return type("C", (WeightGradients,), switches)


def _vae(Z=50, pad=False, W2=784, R1=512, R2=256, G1=256, G2=512):
    """The seven layers' (M, N, lda, ldb, has_bias); pad: the bf16 latent pitch."""
    Zp = (Z + 7) // 8 * 8 if pad else Z
    return [(W2, R1, W2, R1, True), (R1, R2, R1, R2, True), (R2, Z, R2, Zp, True),
            (R2, Z, R2, Zp, True), (Z, G1, Zp, G1, True), (G1, G2, G1, G2, True),
            (G2, W2, G2, W2, True)]


def _plan_vae(K, kind="fp32", collecting=False, Z=50, **switches):
    c = _consts(**switches)
    return plan_wgrads(_vae(Z, pad=kind == "bf16"), K, kind, collecting,
                       kind == "bf16" or c.VAE_WGRAD_X3, c, x3_tn=VAE_X3_TN)


ALL7 = tuple(range(7))


def test_vae_tall_forms():
    assert WeightGradients.WGRAD_TN_X3_SPLITS == 16 and WeightGradients.WGRAD_TN_SPLITS == 8
    assert _plan_vae(24576) == [WgradLaunch(TALL_X3, ALL7, 16)]
    assert _plan_vae(24576, "bf16") == [WgradLaunch(TALL_BF16, ALL7, 8)]
    # the VAE goes tall while the small-batch group collects (AIR, B = 768)
    assert _plan_vae(2304, collecting=True) == [WgradLaunch(TALL_X3, ALL7, 16)]
    assert _plan_vae(2047, collecting=True) == [WgradLaunch(GROUP, ALL7, 0)]


def test_vae_small_batch():
    assert _plan_vae(192, collecting=True) == [WgradLaunch(GROUP, ALL7, 0)]
    # group off: rec_mean + rec_log_variance batched, K // 256 = 0 -> split 1
    assert _plan_vae(192) == [WgradLaunch(SPLITK_F32, m, 1)
                              for m in ((0,), (1,), (2, 3), (4,), (5,), (6,))]
    # bf16 operands are never collected: one bf16 split-K launch per layer
    plan = _plan_vae(192, "bf16", collecting=True)
    assert [(p.form, p.members) for p in plan] == [(SPLITK_BF16, (i,)) for i in range(7)]
    assert all(p.splits == 1 for p in plan)
    # 1024 rows (AIR-ASR's per-step gradients at B = 1024): min(4, ...) fp32, min(2, ...) bf16
    assert [p.splits for p in _plan_vae(1024)] == [4] * 6
    assert [p.splits for p in _plan_vae(1024, "bf16")] == [2] * 7


def test_vae_without_x3():
    plan = _plan_vae(24576, VAE_WGRAD_X3=False)
    assert [(p.form, p.members) for p in plan] == [
        (SPLITK_F32, m) for m in ((0,), (1,), (2, 3), (4,), (5,), (6,))]
    # recognition_1, 784 x 512: 13 x 8 = 104 tiles, ceil(2048 / 104) = 20
    assert plan[0].splits == 20


def test_vae_odd_latent_takes_in_gemm_x3():
    """Z = 25: no tall launch (all-or-nothing evenness); the four
    16-byte-row layers split inside the GEMM, the rest on fp32 split-K."""
    plan = _plan_vae(24576, Z=25)
    assert [(p.form, p.members) for p in plan] == [
        (X3_TN, (0,)), (X3_TN, (1,)), (SPLITK_F32, (2, 3)), (SPLITK_F32, (4,)), (X3_TN, (5,)),
        (X3_TN, (6,))]
    # 784 x 512 in 128 x 128 tiles: 7 x 4 = 28, ceil(512 / 28) = 19
    assert plan[0].splits == 19
    # below X3_MIN_ROWS the in-GEMM form is off too; the group collects them
    assert _plan_vae(192, Z=25, collecting=True) == [WgradLaunch(GROUP, ALL7, 0)]


def _plan_air_heads(TB, collecting, H=256, HS=64):
    """AIRModel._weight_grads_heads' hidden layers; the tall form takes
    mog_heads_output_wgrad for the output layers with it, any other the
    planner again (1-column layers, then 2-column ones)."""
    hidden = plan_wgrads([(H, HS, H, 5 * HS, True)] * 5, TB, "fp32", collecting, HS < 128,
                         WeightGradients, group_first=True)
    if hidden[0].form == TALL_X3:
        return hidden, "heads_output_wgrad"
    return hidden, plan_wgrads([(HS, 1, HS, 2, True)] * 3 + [(HS, 2, HS, 2, True)] * 2, TB,
                               "fp32", collecting, False, WeightGradients)


def test_air_heads_prefer_the_group():
    five = tuple(range(5))
    assert _plan_air_heads(2304, True) == ([WgradLaunch(GROUP, five, 0)],
                                           [WgradLaunch(GROUP, five, 0)])
    assert _plan_air_heads(2304, False) == ([WgradLaunch(TALL_X3, five, 16)],
                                            "heads_output_wgrad")
    hidden, outs = _plan_air_heads(192, False)
    assert [(p.form, p.members) for p in hidden] == [(SPLITK_F32, five)]
    assert [(p.form, p.members) for p in outs] == [(SPLITK_F32, (0, 1, 2)), (SPLITK_F32, (3, 4))]


def test_recurrent_rows():
    air = [(256, 1024, 256, 1024, False)]
    for collecting in (False, True):  # tall from 2048 rows, group or not
        assert plan_wgrads(air, 2048, "fp32", collecting, True, WeightGradients) == [
            WgradLaunch(TALL_X3, (0,), 16)]
    assert plan_wgrads(air, 1536, "fp32", True, True, WeightGradients) == [
        WgradLaunch(GROUP, (0,), 0)]
    # 4 x 16 tiles: ceil(2048 / 64) = 32 > 1536 // 256 = 6
    assert plan_wgrads(air, 1536, "fp32", False, True, WeightGradients) == [
        WgradLaunch(SPLITK_F32, (0,), 6)]
    assert plan_wgrads(air, 16384, "fp32", False, False, WeightGradients)[0].form == SPLITK_F32
    # carried as it was: the recurrent rows go tall without the evenness check
    # (an odd rnn_units is the tall kernel's invalid-argument error, no fallback)
    odd = [(255, 1020, 255, 1020, False)]
    assert plan_wgrads(odd, 2048, "fp32", False, True, WeightGradients, check_even=False) == [
        WgradLaunch(TALL_X3, (0,), 16)]
    assert plan_wgrads(odd, 2048, "fp32", False, True, WeightGradients)[0].form == SPLITK_F32
    # AIR-ASR's two cells: one tall launch; else two launches (one has a bias)
    asr = [(312, 1024, 312, 1024, False), (312, 1024, 312, 1024, True)]
    assert plan_wgrads(asr, 3072, "fp32", True, True, WeightGradients) == [
        WgradLaunch(TALL_X3, (0, 1), 16)]
    assert plan_wgrads(asr, 1024, "fp32", False, True, WeightGradients) == [
        WgradLaunch(SPLITK_F32, (0,), 4), WgradLaunch(SPLITK_F32, (1,), 4)]


def test_one_pass_leaves_the_tall_splits():
    one = dict(ONE_PASS_WGRADS=True)
    assert _plan_vae(24576, **one) == [WgradLaunch(TALL_X3, ALL7, 16)]
    assert _plan_vae(24576, "bf16", **one) == [WgradLaunch(TALL_BF16, ALL7, 8)]
    for plan in (_plan_vae(24576, VAE_WGRAD_X3=False, **one), _plan_vae(24576, Z=25, **one),
                 _plan_vae(1024, "bf16", **one)):
        assert plan and all(p.splits == 1 for p in plan)


def test_equal_neighbours_share_a_launch():
    """Consecutive problems of one (M, N, lda, ldb, has_bias) share a batched
    split-K launch wherever they occur, and its split count counts their
    tiles together: with recognition units (256, 256) and Z = 256 the VAE's
    recognition_2, rec_mean, rec_log_variance and generative_1 (all 256 x
    256) are one launch (4 x 4 tiles x 4: ceil(2048 / 64) = 32, K // 256 = 8
    at 2048 rows)."""
    shapes = _vae(Z=256, R1=256, R2=256)
    plan = plan_wgrads(shapes, 2048, "fp32", False, False, WeightGradients, x3_tn=VAE_X3_TN)
    assert [(p.form, p.members) for p in plan] == [
        (SPLITK_F32, m) for m in ((0,), (1, 2, 3, 4), (5,), (6,))]
    assert plan[1].splits == 8 and plan[0].splits == 8  # (13 x 4 tiles: ceil(2048 / 52) = 40)
    # a neighbour of the same extents without a bias starts its own launch
    pair = [(64, 64, 64, 64, True), (64, 64, 64, 64, False), (64, 64, 64, 64, False)]
    assert [p.members for p in plan_wgrads(pair, 192, "fp32", False, False, WeightGradients)] == [
        (0,), (1, 2)]


def _run_executor(monkeypatch, shapes, K, collecting=False, **kw):
    """WeightGradients._wgrads on named stand-ins for the tensors, the ops
    replaced by recorders: the (tag, work) pairs it times and the calls."""
    import contextlib

    from mog_air import wgrads
    tags, calls = [], []

    class Group:
        def add(self, *a):
            calls.append(("group.add",) + a)

    class Model(WeightGradients):
        _wgroup = Group() if collecting else None

        def _timed(self, name, work=None):
            tags.append((name, work))
            return contextlib.nullcontext()

    def recorder(name):
        return lambda *a, **k: calls.append((name, a, k))
    for name in ("wgrad_tn_x3", "wgrad_tn_bf16", "gemm_x3_tn"):
        monkeypatch.setattr(wgrads.ops, name, recorder(name))
    for name in ("gemm", "gemm_bf16"):
        monkeypatch.setattr(wgrads, name, recorder(name))
    probs = [wgrads.WgradProblem("X%d" % i, "dY%d" % i, "out%d" % i, "b%d" % i if bias else None,
                                 M, N, lda, ldb) for i, (M, N, lda, ldb, bias) in enumerate(shapes)]
    Model()._wgrads(probs, K, **kw)
    return tags, calls


def test_executor_tags_flops_and_arguments(monkeypatch):
    """The executor's _timed tags and flop amounts (bench.py prices them by
    tag) and the arguments it hands the ops."""
    vae = dict(tag="vae_wgrad_x3", tall=True, x3_tn=VAE_X3_TN)
    flops = [2.0 * M * N for M, N, *_ in _vae()]
    # tall x3: one launch, the seven layers' flops, dims (M, N, lda, ldb, N)
    tags, calls = _run_executor(monkeypatch, _vae(), 24576, **vae)
    assert tags == [("vae_wgrad_x3", ("mfma", 24576 * sum(flops), "fp32", "x3"))]
    (name, a, _), = calls
    assert name == "wgrad_tn_x3" and a[0] == ["X%d" % i for i in range(7)]
    assert a[3] == ["b%d" % i for i in range(7)] and a[5:] == (24576, 16)
    assert a[4] == [(M, N, lda, ldb, N) for M, N, lda, ldb, _ in _vae()]
    # bf16: the tall launch under the call site's tag, the split-K ones as wgrad_bf16
    bf = dict(tag="vae_wgrad_bf16", tall=True, kind="bf16")
    tags, calls = _run_executor(monkeypatch, _vae(pad=True), 24576, **bf)
    assert tags == [("vae_wgrad_bf16", ("mfma", 24576 * sum(flops), "bf16"))]
    assert calls[0][0] == "wgrad_tn_bf16" and calls[0][1][5:] == (24576, 8)
    tags, calls = _run_executor(monkeypatch, _vae(pad=True), 192, **bf)
    assert tags == [("wgrad_bf16", ("mfma", 192 * f, "bf16")) for f in flops]
    assert [c[0] for c in calls] == ["gemm_bf16"] * 7 and calls[2][2]["colsum"] == ["b2"]
    assert calls[2][1][6:] == (256, 56, 50) and calls[2][2]["splitk"] == 1  # lda, ldb, ldc
    # fp32 split-K: wgrad_f32, a batched launch priced for its members
    tags, calls = _run_executor(monkeypatch, _vae(), 192, **vae)
    assert [t for t, _ in tags] == ["wgrad_f32"] * 6
    assert tags[2] == ("wgrad_f32", ("mfma", 192 * (flops[2] + flops[3]), "fp32"))
    name, a, k = calls[2]
    assert name == "gemm" and a[:3] == (["X2", "X3"], ["dY2", "dY3"], ["out2", "out3"])
    assert a[3:] == (256, 50, 192, 256, 50, 50) and k["colsum"] == ["b2", "b3"]
    assert k["transA"] is True and k["splitk"] == 1
    # in-GEMM x3 (odd latent): the call site's tag, float atomics (reduce=False)
    tags, calls = _run_executor(monkeypatch, _vae(Z=25), 24576, **vae)
    assert [t for t, _ in tags] == ["vae_wgrad_x3", "vae_wgrad_x3", "wgrad_f32", "wgrad_f32",
                                    "vae_wgrad_x3", "vae_wgrad_x3"]
    assert tags[0][1] == ("mfma", 24576 * flops[0], "fp32", "x3")
    assert calls[0][0] == "gemm_x3_tn" and calls[0][2] == dict(splitk=19, colsum="b0", reduce=False)
    # collected: no launch, no tag; a problem without a bias passes None
    tags, calls = _run_executor(monkeypatch, [(256, 1024, 256, 1024, False)], 1536,
                                collecting=True, tag="rec_wgrad_x3", tall=True, check_even=False)
    assert tags == [] and calls == [("group.add", "X0", "dY0", "out0", 256, 1024, 1536, 256, 1024,
                                     1024, None)]
    tags, calls = _run_executor(monkeypatch, [(256, 1024, 256, 1024, False)], 2048,
                                collecting=True, tag="rec_wgrad_x3", tall=True, check_even=False)
    assert [t for t, _ in tags] == ["rec_wgrad_x3"] and calls[0][1][3] == [None]
