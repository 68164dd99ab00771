"""AIR cnn=True on the device: the encoder's two ops against the restated
encoder (tests/air_cnn_ref.py; forward bit for bit, backward against float64
autograd), then the model with the encoder ahead of its LSTM -- forward,
gradients, train steps, the captured step, generation and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle import air_torch as at

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_cnn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _max_ipw():
    """The most images one workgroup of the backward sums (what a large
    batch uses)."""
    from mog_air import ops
    return ops.cnn_images_per_wg(1 << 30)


def _multi_wg_batch():
    """Several workgroups of the backward at _max_ipw() images each, with a
    ragged last one."""
    return min(2 * _max_ipw() + 1, 130)


_OP_CASES = {}


def _op_case(B):
    """Canvases (the last one with content in every corner and on the
    pooling seams), the encoder's tensors, dF, and the float64 gradients of
    <dF, features> -- computed once per batch size."""
    if B in _OP_CASES:
        return _OP_CASES[B]
    P = ref.cnn_params(3300 + B)
    x = ao.synthetic_canvases(B, seed=300)[0]
    x[-1] = ref.corner_canvas()
    dF = np.random.default_rng(40 + B).standard_normal((B, ref.NFEAT)).astype(np.float32)
    Pt = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in P.items()}
    (ref.encoder_torch(x, Pt) * torch.tensor(dF, dtype=torch.float64)).sum().backward()
    c = dict(P=P, x=x, dF=dF, feat=ref.encoder_numpy(x, P),
             grads={n: Pt[n].grad.numpy() for n in ref.cnn_names()})
    _OP_CASES[B] = c
    return c


def _run_forward(c):
    from mog_air import ops
    B = c["x"].shape[0]
    w = [_cuda(c["P"][n]) for n in ref.cnn_names()]
    e = lambda n: torch.full((B, n), float("nan"), device=DEV)  # noqa: E731
    pool1, pool2, feat = e(625 * 8), e(ref.NFEAT), e(ref.NFEAT)
    x = _cuda(c["x"])
    ops.cnn_enc_forward(x, w, pool1, pool2, feat)
    return x, w, pool1, pool2, feat


@pytest.mark.parametrize("B", [1, 5, 6, "multi"])
def test_encoder_forward_bit_exact(B):
    B = _multi_wg_batch() if B == "multi" else B
    c = _op_case(B)
    _, _, pool1, pool2, feat = _run_forward(c)
    _, p1, _, p2, _ = ref.encoder_planes(c["x"], c["P"])
    np.testing.assert_array_equal(pool1.cpu().numpy(), p1.reshape(B, -1))
    np.testing.assert_array_equal(pool2.cpu().numpy(), p2.reshape(B, -1))
    np.testing.assert_array_equal(feat.cpu().numpy(), c["feat"])
    share = float((c["feat"] != 0).mean())
    assert 0.2 <= share <= 0.95, share


@pytest.mark.parametrize("B", [1, 5, 6, "multi"])
def test_encoder_backward_vs_float64_autograd_and_deterministic(B):
    from mog_air import ops
    B = _multi_wg_batch() if B == "multi" else B
    c = _op_case(B)
    x, w, pool1, pool2, feat = _run_forward(c)
    dF = _cuda(c["dF"])
    # the multi-workgroup batch at the images per workgroup of a large batch
    # (the default at these sizes is one: test_encoder_backward_images_per_wg)
    ipw = _max_ipw() if B == _multi_wg_batch() else None
    runs = []
    for fill in (float("nan"), 0.0):  # (the gradients are stored, the scratch written first)
        part = torch.full((ops.cnn_partial_elems(B, ipw),), fill, device=DEV)
        grads = [torch.full_like(t, fill) for t in w]
        ops.cnn_enc_backward(x, w, pool1, pool2, feat, dF, part, grads, images_per_wg=ipw)
        runs.append([g.cpu().numpy() for g in grads])
    for name, got, again in zip(ref.cnn_names(), *runs):
        want = c["grads"][name]
        assert np.linalg.norm(want) > 0, name
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"B={B} {name}: relative error {err:.3g}")
        assert err < 1e-5, (name, err)
        np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32), err_msg=name)


def test_encoder_backward_images_per_wg():
    """The default images per workgroup (B / 512 clamped to 1..8) and every
    explicit one on the multi-workgroup batch: the same gradients to the
    reference's bar (the sums only change their order)."""
    from mog_air import ops
    assert [ops.cnn_images_per_wg(b) for b in (1, 64, 1023, 1024, 2048, 4095, 4096, 65536)] == [
        1, 1, 1, 2, 4, 7, 8, 8]
    assert ops.cnn_partial_elems(17) == 17 * 3424 and ops.cnn_partial_elems(17, 8) == 3 * 3424
    B = _multi_wg_batch()
    c = _op_case(B)
    x, w, pool1, pool2, feat = _run_forward(c)
    dF = _cuda(c["dF"])
    for ipw in (None, 2, 3, _max_ipw()):
        part = torch.full((ops.cnn_partial_elems(B, ipw),), float("nan"), device=DEV)
        grads = [torch.full_like(t, float("nan")) for t in w]
        ops.cnn_enc_backward(x, w, pool1, pool2, feat, dF, part, grads, images_per_wg=ipw)
        for name, g in zip(ref.cnn_names(), grads):
            want = c["grads"][name]
            err = np.linalg.norm(g.cpu().numpy() - want) / np.linalg.norm(want)
            assert err < 1e-5, (ipw, name, err)
    with pytest.raises(ValueError):
        ops.cnn_enc_backward(x, w, pool1, pool2, feat, dF, part, grads, images_per_wg=9)


def test_encoder_ops_reject_bad_arguments():
    from mog_air import ops
    c = _op_case(5)
    x, w, pool1, pool2, feat = _run_forward(c)
    with pytest.raises(ValueError):
        ops.cnn_enc_forward(x[:, :2499].contiguous(), w, pool1, pool2, feat)
    with pytest.raises(ValueError):
        ops.cnn_enc_forward(x, w, pool1[:4], pool2, feat)
    with pytest.raises(ValueError):  # the partial sums of a smaller batch
        ops.cnn_enc_backward(x, w, pool1, pool2, feat, torch.zeros_like(feat),
                             torch.zeros(ops.cnn_partial_elems(5) - 1, device=DEV),
                             [torch.zeros_like(t) for t in w])


# ------------------------------------------------------------- model -----
def _model(cfg, P, scope, cnn=True, train=True, **kw):
    from mog_air.air_model import AIRModel
    m = AIRModel(max_steps=cfg.max_steps, canvas_size=cfg.canvas_size,
                 scale_prior_variance=cfg.scale_prior_variance,
                 z_pres_prior_log_odds=cfg.z_pres_prior_log_odds,
                 z_pres_temperature=cfg.z_pres_temperature,
                 stopping_threshold=cfg.stopping_threshold,
                 vae_likelihood_std=cfg.vae_likelihood_std, learning_rate=1e-4,
                 gradient_clipping_norm=1.0, cnn=cnn, train=train, scope=scope, device=DEV, **kw)
    if P is not None:
        m.params.load_dict(P)
    return m


def _noise(nz):
    return {k: _cuda(v) for k, v in nz.items()}


def test_model_forward_features_counts_and_loss_deviation():
    """rnn_input bit for bit, the counts of the float64 loop, and the largest
    relative per-image loss deviation from that loop within 4 d0, d0 being the
    same deviation of a cnn=False model against oracle/air_torch.py.
    Measured on an MI355X: d0 = 0.0817, cnn=True 0.0439."""
    c = ref.case(300, 6)
    ref.check_case(c)
    cfg, x, k = c["cfg"], c["x"], c["k"]
    m = _model(cfg, c["P"], "cnn_fwd")
    m.infer(x, k, noise=_noise(c["nz"]))
    np.testing.assert_array_equal(m.rnn_input.cpu().numpy(), ref.encoder_numpy(x, c["P"]))
    want = ref.reference64(c)
    assert m.executed_steps == want["T"]
    np.testing.assert_array_equal(m.rec_num_digits.cpu().numpy(), want["digits"].numpy())
    dev = np.abs(m.per_image_loss.cpu().numpy() / want["loss_b"].numpy() - 1.0).max()
    # d0: existing code against the existing reference, same images and noise
    m0 = _model(cfg, c["P0"], "cnn_fwd0", cnn=False)
    m0.infer(x, k, noise=_noise(c["nz"]))
    with torch.no_grad():
        want0 = at.air_forward(cfg, at.to_torch(c["P0"]), at.to_torch(c["nz"]),
                               torch.tensor(x, dtype=torch.float64), torch.tensor(k))
    assert m0.executed_steps == want0["T"]
    d0 = np.abs(m0.per_image_loss.cpu().numpy() / want0["loss_b"].numpy() - 1.0).max()
    print(f"per-image loss deviation: cnn=False d0 = {d0:.3g}, cnn=True = {dev:.3g}")
    assert dev <= 4.0 * d0, (dev, d0)


def test_model_gradient_parity_vs_float64_autograd():
    c = ref.case(301, 8)
    ref.check_case(c)
    cfg, x, k = c["cfg"], c["x"], c["k"]
    Gc = (np.random.default_rng(9).standard_normal((cfg.batch, 2500)) * 0.01).astype(np.float32)
    m = _model(cfg, c["P"], "cnn_grad")
    grads = m.compute_gradients(x, k, noise=_noise(c["nz"]), canvas_cotangent=_cuda(Gc))
    Pt = at.to_torch(c["P"], requires_grad=True)
    out = ref.air_cnn_forward_torch(cfg, Pt, at.to_torch(c["nz"]),
                                    torch.tensor(x, dtype=torch.float64),
                                    z_pres_prior_log_odds=cfg.z_pres_prior_log_odds,
                                    canvas_cotangent=torch.tensor(Gc, dtype=torch.float64),
                                    fixed_steps=True)
    out["loss"].backward()
    assert set(grads) == set(Pt)
    for name, p in Pt.items():
        want = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        got = grads[name]
        if name in ref.cnn_names():
            assert np.linalg.norm(want) > 0, name
        err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-12)
        assert err < 2e-3 or np.linalg.norm(got - want) < 1e-6, (name, err)


def _train_model(scope, **kw):
    from mog_air.air_model import AIRModel
    return AIRModel(max_steps=3, max_digits=3, canvas_size=50, scale_prior_variance=0.05,
                    z_pres_prior_log_odds=-0.01, learning_rate=1e-3, gradient_clipping_norm=1.0,
                    cnn=True, train=True, scope=scope, device=DEV, seed=21, noise_seed=22, **kw)


def _data(n, B=64):
    return [tuple(_cuda(a, dt) for a, dt in zip(ao.synthetic_canvases(B, seed=300 + i),
                                                (torch.float32, torch.int32)))
            for i in range(n)]


def test_train_steps_move_the_encoder_and_are_deterministic():
    data = _data(3)
    ma, mb = _train_model("cnn_tr_a"), _train_model("cnn_tr_b")
    start = ma.params.state_dict()
    assert all(np.abs(start[n]).max() > 0 for n in ref.cnn_names() if n.endswith("kernel"))
    for x, k in data:
        loss, acc, mse, gs = ma.step(x, k)
        mb.step(x, k)
        assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    assert gs == 3 and mb.global_step == 3
    end = ma.params.state_dict()
    assert np.all(np.isfinite(ma.params.flat.cpu().numpy()))
    for n in ref.cnn_names():
        assert not np.array_equal(start[n], end[n]), n
    assert torch.equal(ma.params.flat.view(torch.int32), mb.params.flat.view(torch.int32))


def test_graph_replay_matches_eager_bitwise():
    data = _data(2)
    me, mg = _train_model("cnn_g_e"), _train_model("cnn_g_g")
    for x, k in data:
        me.train_step_async(x, k)
        mg.train_step_graphed(x, k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(me._ws.means[:3].cpu().numpy(),
                                      mg._ws.means[:3].cpu().numpy())
    assert mg._graph is not None and me.global_step == mg.global_step == 2
    assert torch.equal(me.params.flat.view(torch.int32), mg.params.flat.view(torch.int32))


def test_generation_does_not_depend_on_the_encoder():
    cfg = ao.AirConfig(max_steps=3)
    mc = _model(cfg, None, "cnn_gen_c", train=False, seed=5, noise_seed=6)
    mf = _model(cfg, None, "cnn_gen_f", cnn=False, train=False, seed=7, noise_seed=6)
    shared = {n: v for n, v in mc.params.state_dict().items()
              if n != ref.KERNEL and not n.startswith(ref.CNN)}
    assert len(shared) == len(mf.params.specs) - 1
    mf.params.load_dict(shared)
    a = mc.generate(3, batch=16).cpu().numpy()
    b = mf.generate(3, batch=16).cpu().numpy()
    assert a.shape == (16, 50, 50, 1) and a.max() > 0
    np.testing.assert_array_equal(a, b)


def test_refusals():
    from mog_air.air_model import AIRModel
    from mog_air.asr_model import AIRModel as AsrModel
    kw = dict(max_steps=3, train=True, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        AIRModel(cnn=True, precision="bf16", scope="cnn_r1", **kw)
    with pytest.raises(ValueError, match="canvas"):
        AIRModel(cnn=True, canvas_size=64, scope="cnn_r2", **kw)
    with pytest.raises(NotImplementedError, match="cnn_filters"):
        AIRModel(cnn=True, cnn_filters=4, scope="cnn_r3", **kw)
    with pytest.raises(NotImplementedError):  # the AIR-ASR model's refusal stays
        AsrModel(None, None, cnn=True, scope="cnn_r4", **kw)
    m = AIRModel(cnn=True, scope="cnn_r5", **kw)

    class Reducer:
        def launch(self, view):
            raise AssertionError("no bucket may be handed over")

        def wait(self):
            pass

    x, k = _data(1, 8)[0]
    m.grad_reducer = Reducer()
    with pytest.raises(NotImplementedError, match="single-device"):
        m.train_step_async(x, k)
    m.grad_reducer = None
    m.live_hook = lambda live, t: None
    with pytest.raises(NotImplementedError, match="single-device"):
        m.infer(x, k)
    m.live_hook = None
    m.step(x, k)  # and the model still trains once they are detached
    assert m.global_step == 1


def test_entry_point_trains_with_cnn(tmp_path, monkeypatch):
    """training_air_original.py --cnn 1: offline synthetic data, a few
    iterations, the final evaluation."""
    import glob

    import training_air_original as entry
    monkeypatch.chdir(tmp_path)  # results/ and data/ paths are relative, as in the reference
    step = entry.main(["-dn", "13", "-data", "mnist", "-r", str(tmp_path / "res"), "-k", "t",
                       "--iterations", "21", "--synth-per-count", "40", "--cnn", "1"])
    assert step == 21
    text = open(glob.glob(str(tmp_path / "res_(t)" / "logfile*.log"))[0]).read()
    assert "iteration 20\ttrain loss" in text and "iteration final\ttest loss" in text


def test_b1024_side_streams_and_presplit_x_rows_match_the_serial_chain():
    """B = 1024: the step forks its side streams (SIDE_MIN_BATCH), the x-rows
    gradient takes the pre-split three-piece form on the features (from
    X3P_MIN_B = 256) and a workgroup of the encoder backward sums two images.
    Against the same model with every fork off and the fp32 chain: forward and
    the encoder's gradients bit for bit (dF and the encoder's sums do not
    depend on either), the rest within the split forms' tolerance
    (tests/test_gpu_graph.py's)."""
    from mog_air import ops
    B = 1024
    assert ops.cnn_images_per_wg(B) == 2
    (x, k), = _data(1, B)
    mp, ms = _train_model("cnn_sd_p"), _train_model("cnn_sd_s")
    ms.HEADS_WGRAD_SIDE = ms.REC_WGRAD_SIDE = ms.NOISE_ON_SIDE = False
    ms.X_GRAD_X3 = 0
    assert mp._x3p_xgrad(B) and not ms._x3p_xgrad(B) and B >= mp.SIDE_MIN_BATCH
    for m in (mp, ms):
        m.ONE_PASS_WGRADS = True
    gp, gs = mp.compute_gradients(x, k), ms.compute_gradients(x, k)
    np.testing.assert_array_equal(mp._ws.means[:3].cpu().numpy(), ms._ws.means[:3].cpu().numpy())
    np.testing.assert_array_equal(mp.rnn_input.cpu().numpy(), ms.rnn_input.cpu().numpy())
    bad = []
    for name in gs:
        a, b = gs[name], gp[name]
        if name in ref.cnn_names():
            assert np.abs(a).max() > 0, name
            np.testing.assert_array_equal(a, b, err_msg=name)
            continue
        err, scale = float(np.abs(a - b).max()), float(np.abs(a).max())
        if err > (1e-2 if a.size <= 64 else 1e-3) * max(scale, 1e-30):
            bad.append((name, err, scale))
    assert not bad, bad[:5]
