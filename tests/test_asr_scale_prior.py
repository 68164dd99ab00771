"""AIR-ASR learned scale prior (fix_scale_distribution=False), CPU side: the
test helper (tests/asr_scale_prior_ref.py) pinned to the oracle where the two
overlap (the fixed prior), its inputs shown not to be degenerate, and the
parameter table with the gen_scale block."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import asr_oracle as so
from oracle import asr_torch as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asr_scale_prior_ref as ref  # noqa: E402


@pytest.mark.parametrize("k", sorted(ref.SETS))
def test_numpy_restatement_equals_oracle_with_fixed_prior(k):
    c = ref.case(k)
    ref.check_case(c)
    o = c["ref"]
    for name in ("fixed", "learned"):  # the prior moves neither scale nor shift
        np.testing.assert_array_equal(c[name]["scale"], o["scale"])
        np.testing.assert_array_equal(c[name]["shift"], o["shift"])
    np.testing.assert_array_equal(c["fixed"]["scale_kl"], o["scale_kl"])
    # activity restated from z_pres is the oracle's own: its masked KLs vanish there only
    np.testing.assert_array_equal(c["fixed"]["act"], o["scale_kl"] != 0)


@pytest.mark.parametrize("kw", [dict(fix_steps=2), dict(train=False)])
def test_numpy_restatement_equals_oracle_variants(kw):
    ref.check_case(ref.case(1))
    c = ref.case(1, **kw)
    assert c["ref"]["T"] >= 2
    np.testing.assert_array_equal(c["fixed"]["scale"], c["ref"]["scale"])
    np.testing.assert_array_equal(c["fixed"]["scale_kl"], c["ref"]["scale_kl"])


def _grads(fn, P):
    Pt = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in P.items()}
    out = fn(Pt)
    out["loss"].backward()
    return out, Pt


@pytest.mark.parametrize("fix", [None, 2])
def test_torch_restatement_equals_oracle_with_fixed_prior(fix):
    ref.check_case(ref.case(1))
    c = ref.case(1, fix_steps=fix)
    cfg, nz = c["cfg"], c["nz"]
    x = torch.tensor(c["x"], dtype=torch.float64).reshape(cfg.batch, -1)
    Gc = torch.tensor(np.random.default_rng(31).standard_normal((cfg.batch, 2500)) * 0.01)
    want, Pw = _grads(lambda P: st.asr_forward(cfg, P, nz, x, canvas_cotangent=Gc), c["P_fixed"])
    got, Pg = _grads(lambda P: ref.asr_loss_torch(cfg, P, nz, x, Gc, False), c["P_fixed"])
    assert got["T"] == want["T"] == 4
    assert float(got["loss"]) == pytest.approx(float(want["loss"]), rel=1e-12)
    for n in Pw:
        if Pw[n].grad is None:
            assert Pg[n].grad is None, n
            continue
        np.testing.assert_allclose(Pg[n].grad.numpy(), Pw[n].grad.numpy(), rtol=1e-12,
                                   atol=1e-12 * float(Pw[n].grad.abs().max()), err_msg=n)


def test_torch_restatement_learned_prior_reaches_the_new_tensors():
    c = ref.case(1)
    ref.check_case(c)
    cfg, nz = c["cfg"], c["nz"]
    x = torch.tensor(c["x"], dtype=torch.float64).reshape(cfg.batch, -1)
    Gc = torch.tensor(np.random.default_rng(31).standard_normal((cfg.batch, 2500)) * 0.01)
    _, Pl = _grads(lambda P: ref.asr_loss_torch(cfg, P, nz, x, Gc, True), c["P"])
    _, Pf = _grads(lambda P: ref.asr_loss_torch(cfg, P, nz, x, Gc, False), c["P"])
    for n, _ in ref.gen_scale_specs(cfg):
        assert float(Pl[n].grad.abs().max()) > 0, n
        assert Pf[n].grad is None
    # through shift_latent the prior's gradient reaches the inference shift
    # heads, through hg the generative LSTM; the gen_shift heads see neither:
    # their gradient is hg^T d(shift KL), and the flag moves no forward value
    for n in ("inf_shift/dense/kernel", "inf_shift/dense_3/bias", "gen_rnn_running/kernel"):
        n = so.P_ROOT + n
        assert not np.array_equal(Pl[n].grad.numpy(), Pf[n].grad.numpy()), n
    n = so.P_ROOT + "gen_shift/dense/kernel"
    np.testing.assert_array_equal(Pl[n].grad.numpy(), Pf[n].grad.numpy())


def test_param_specs_append_the_gen_scale_block():
    from mog_air.asr_model import asr_param_specs
    args = (2500, 256, 784, (512, 256), (256, 512), 50, 64, 64)
    cfg = so.AsrConfig()
    fixed = asr_param_specs(*args)
    assert fixed == so.param_specs(cfg) == asr_param_specs(*args, False)
    learned = asr_param_specs(*args, True)
    assert learned[:len(fixed)] == fixed
    assert learned[len(fixed):] == ref.gen_scale_specs(cfg)
    p = so.P_ROOT + "gen_scale/"
    assert learned[-8:] == [(p + "dense/kernel", (258, 64)), (p + "dense/bias", (64,)),
                            (p + "dense_1/kernel", (66, 1)), (p + "dense_1/bias", (1,)),
                            (p + "dense_2/kernel", (258, 64)), (p + "dense_2/bias", (64,)),
                            (p + "dense_3/kernel", (66, 1)), (p + "dense_3/bias", (1,))]
