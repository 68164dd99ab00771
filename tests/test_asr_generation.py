"""AIR-ASR generation (air_number_bbox_location.py:1124-1361,
vae.py:51-86): known-answer properties of the numpy restatement
(tests/asr_gen_ref.py) on the CPU, and on the GPU the HIP path
(asr_model.AIRModel.generate: generative LSTMCell + asr_gen_step_ + fp32
decoder GEMMs + bernoulli_threshold_ + STN write accumulate) bit-exact against
it on injected noise, the threshold kernel alone, device noise, the image
grids and the train_air_pr.py entry point."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import asr_oracle as so

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asr_gen_ref as ref  # noqa: E402
from test_visualize import _read_png  # noqa: E402

W2 = 784
# k -> (max_steps, generation batch, fix_steps)
CASES = {1: (3, 5, 2), 2: (3, 6, 1), 3: (4, 17, None), 4: (3, 64, None)}


def _cfg(T, G, fix):
    return so.AsrConfig(batch=G, max_steps=T, train=False, z_pres_temperature=1.0,
                        vae_likelihood_std=0.3, stopping_threshold=0.9,
                        constrains_area_minmax=(17.0, 23.0), fix_steps=fix)


@functools.lru_cache(maxsize=None)
def _case(k):
    """(cfg, params, noise, reference result) of case k: computed once, shared
    and left unchanged by the tests."""
    T, G, fix = CASES[k]
    cfg = _cfg(T, G, fix)
    P = so.init_params(cfg, seed=20 + k, bias_scale=0.05)
    nz = so.make_noise(cfg, seed=30 + k)
    nz["u_x"] = np.random.default_rng(30 + k).uniform(0, 1, (T, G, W2)).astype(np.float32)
    out = ref.generate(cfg, P, nz, G)
    for v in list(P.values()) + list(nz.values()) + [a for a in out.values()
                                                     if isinstance(a, np.ndarray)]:
        v.setflags(write=False)
    return cfg, P, nz, out


# ------------------------------------------------------------------ CPU ---
def test_ref_fix_steps_known_answers():
    cfg, _, _, out = _case(2)  # fix_steps=1, max_steps=3
    # step 0 writes (+100), step 1 stops every image (-100): the loop exits
    assert out["T"] == 2 and out["st_back"].shape == (2, 6, 6)
    assert np.all(out["digits"] == 1)
    assert np.all(out["z_pres"][0] == 1) and np.all(out["z_pres"][1] == 0)
    assert not out["act"][1].any()
    # the canvas is step 0's written window; step 1 contributes nothing
    np.testing.assert_array_equal(out["canvas"], out["recon"][0])
    assert out["canvas"].max() > 0


@pytest.mark.parametrize("k", sorted(CASES))
def test_ref_ranges(k):
    cfg, _, _, out = _case(k)
    T = cfg.max_steps
    assert np.isfinite(out["canvas"]).all()
    # (the half-degenerate border samples keep the STN's ~1e-6 cancellation residue)
    assert out["canvas"].min() >= -1e-5 and out["canvas"].max() <= T + 1e-5
    assert np.all((out["windows"] == 0) | (out["windows"] == 1))
    assert 0 < out["windows"].mean() < 1
    assert np.all(1.0 / out["st_back"][..., 0] == np.float32(20 / 50))
    assert np.all((out["digits"] >= 0) & (out["digits"] <= out["T"]))


def test_ref_expected_step_counts():
    assert _case(1)[3]["T"] == 3 and np.all(_case(1)[3]["digits"] == 2)
    assert _case(2)[3]["T"] == 2 and np.all(_case(2)[3]["digits"] == 1)


def _check_learned_prior_reference(out):
    """A degenerate reference (every image alike, nothing written) cannot pass."""
    assert len(np.unique(out["digits"])) >= 3
    assert np.any(out["z_pres"][0] == 0)
    assert out["canvas"].max() > 0


@pytest.mark.parametrize("k", [3, 4])
def test_ref_learned_prior_is_not_degenerate(k):
    _check_learned_prior_reference(_case(k)[3])


# ------------------------------------------------------------------ GPU ---
def _model(T, G, fix, scope, **kw):
    from mog_air.asr_model import AIRModel
    return AIRModel(max_steps=T, cnn=False, train=False, z_pres_temperature=1.0,
                    vae_likelihood_std=0.3, stopping_threshold=0.9,
                    constrains_area_minmax=(17, 23), fix_steps=fix, generation_batch_size=G,
                    scope=scope, device="cuda:0", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(CASES))
def test_hip_generation_matches_reference(k):
    import torch
    T, G, fix = CASES[k]
    cfg, P, nz, out = _case(k)
    if fix is None:
        _check_learned_prior_reference(out)
    m = _model(T, G, fix, f"asrgen{k}")
    m.params.load_dict(P)
    got = m.generate(noise={n: torch.as_tensor(np.array(v)).cuda() for n, v in nz.items()})
    assert got is m.generated_samples and tuple(got.shape) == (G, 50, 50, 1)
    canvas = got.reshape(G, -1).cpu().numpy()
    st = m.generated_st_back.cpu().numpy()
    digits = m.generated_num_digits.cpu().numpy()
    print(f"case {k}: executed {st.shape[1]} (ref {out['T']}), counts "
          f"{np.bincount(digits, minlength=T + 1)} (ref "
          f"{np.bincount(out['digits'], minlength=T + 1)}), canvas mismatches "
          f"{int((canvas != out['canvas']).sum())}")
    assert st.shape == (G, out["T"], 2, 3)
    np.testing.assert_array_equal(st, out["st_back"].transpose(1, 0, 2).reshape(G, -1, 2, 3))
    assert digits.dtype == np.int32
    np.testing.assert_array_equal(digits, out["digits"])
    np.testing.assert_array_equal(canvas, out["canvas"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, W2 * 5, W2 * 5 + 2])
def test_bernoulli_threshold_kernel(n):
    import torch
    import mog_air.ops  # noqa: F401  (registers torch.ops.mog_air)
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g)
    u = torch.rand(n, generator=g)
    u[::3] = x[::3]  # equal pairs give 0 (strict >), vector body and scalar tail alike
    u[-1] = x[-1]
    x, u = x.cuda(), u.cuda()
    out = torch.full((n + 4,), -7.0, device="cuda:0")
    torch.ops.mog_air.bernoulli_threshold_(x, u, out, n)
    want = (x > u).float()
    assert want.sum() > 0 or n < 4
    np.testing.assert_array_equal(out[:n].cpu().numpy(), want.cpu().numpy())
    assert np.all(out[::3][: (n + 2) // 3].cpu().numpy() == 0)
    assert np.all(out[n:].cpu().numpy() == -7.0)  # nothing past n is written
    if n > 4:
        # rows that are not 16-byte aligned take the scalar form: same values
        out2 = torch.full((n,), -7.0, device="cuda:0")
        torch.ops.mog_air.bernoulli_threshold_(x[1:], u[1:], out2[1:], n - 1)
        np.testing.assert_array_equal(out2[1:].cpu().numpy(), want[1:].cpu().numpy())
        assert float(out2[0]) == -7.0


@pytest.mark.gpu
def test_hip_generation_device_noise():
    m = _model(3, 64, None, "asrgen_dev", precision="bf16")
    a = m.generate().cpu().numpy().copy()
    assert a.shape == (64, 50, 50, 1) and np.isfinite(a).all() and a.max() > 0
    d = m.generated_num_digits.cpu().numpy()
    assert np.all((d >= 0) & (d <= 3))
    assert m.generated_st_back.shape[0] == 64 and 1 <= m.generated_st_back.shape[1] <= 3
    b = m.generate().cpu().numpy()
    assert not np.array_equal(a, b)  # the Philox counter advanced


@pytest.mark.gpu
def test_generation_rejects_non_positive_write_scale():
    from mog_air.asr_model import AIRModel
    m = AIRModel(max_steps=2, cnn=False, train=False, scope="asrgen_bad", device="cuda:0")
    with pytest.raises(ValueError, match="positive"):
        m.generate()


@pytest.mark.gpu
def test_asr_generation_grids(tmp_path):
    from oracle import air_oracle as ao
    from mog_air import visualize as V
    m = _model(3, 64, None, "asrgen_vis")
    x, k = ao.synthetic_canvases(16, seed=3)
    V.save_visualizations(m, x, k, str(tmp_path), 7, digits=None, num=9)
    gen = _read_png(str(tmp_path / "visualize_gen7.png"))
    box = _read_png(str(tmp_path / "visualize_genbbox7.png"))
    # 64 canvases -> 8 x 8 grid of [C, C] and of 2x enlarged [2C, 2C] panels
    assert gen.shape == (8 * 50, 8 * 50, 3) and box.shape == (8 * 100, 8 * 100, 3)
    assert gen.max() > 0
    assert _read_png(str(tmp_path / "visualize_7.png")).shape == (3 * 100, 3 * 208, 3)
    # gen_tag names the generation pair alone (the trainer's final dump)
    V.save_visualizations(m, x, k, str(tmp_path), "final", digits=None, num=9, gen_tag=21)
    assert (tmp_path / "visualize_final.png").exists()
    assert (tmp_path / "visualize_gen21.png").exists()
    assert (tmp_path / "visualize_genbbox21.png").exists()


@pytest.mark.gpu
def test_train_air_pr_writes_generation_grids(tmp_path, monkeypatch):
    import train_air_pr as entry
    monkeypatch.chdir(tmp_path)
    step = entry.main(["-dn", "13", "-gm", "100", "-gne", "10", "-r", str(tmp_path / "res"), "-k",
                       "g", "--iterations", "21", "--synth-per-count", "40"])
    assert step == 21
    summary = tmp_path / "res_(g)" / "summary"
    for name in ("visualize_gen21.png", "visualize_genbbox21.png"):
        img = _read_png(str(summary / name))
        assert img.ndim == 3 and img.shape[2] == 3 and img.size > 0
