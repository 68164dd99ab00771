"""tests/asr_log_row_ref.py (the float64 restatement of the AIR-ASR log row)
against the expressions of asr_model.AIRModel.log_variables, evaluated by CPU
torch in fp32 on crafted arrays: the restatement sums what the property sums,
within bar (b) -- the forward error of the property's own fp32 reductions."""
import numpy as np
import pytest
import torch

import asr_log_row_ref as ref

T = 6


def _property(a):
    """log_variables' reductions (asr_model.py: _records(k).sum(1).mean(), ...)
    on CPU tensors, in its order."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in a.items()}
    tx = int(t["live"][:T].sum())
    records = lambda q: t["arec"][:, q][:tx].transpose(0, 1)  # noqa: E731  (_bt)
    m = lambda v: float(v.mean())  # noqa: E731
    kls = {k: float(records(ref.SLOTS[k]).sum(1).mean())
           for k in ("z_pres_kl", "scale_kl", "shift_kl")}
    return {"z_pres_kl": kls["z_pres_kl"], "scale_kl": kls["scale_kl"],
            "shift_kl": kls["shift_kl"],
            "vae_kl": float((t["vkl"] * t["zmask"])[:tx].sum(0).mean()),
            "pr_num": float(records(ref.SLOTS["pr_num"]).sum(1).mean()),
            "recon": m(t["bce"]), "mse": m(t["mse"]), "area_loss": m(t["area"]),
            "out_loss": m(t["outl"]), "size_loss": m(t["size"]), "over_loss": m(t["over"]),
            "num_margin": float(t["margin"][0]), "num_min_KL": m(t["element"]),
            "TotLoss": float(t["means"][0]), "elbo": m(t["klsum"] + t["bce"]),
            "accu": float(t["means"][1])}


@pytest.mark.parametrize("B", [1, 5, 67, 1030])
@pytest.mark.parametrize("t_exec", [1, 3, 6])
def test_restatement_matches_the_property_expressions(B, t_exec):
    a = ref.crafted(T, t_exec, B, seed=100 * B + t_exec)
    want = _property(a)
    assert tuple(want) == ref.NAMES
    row, bar = ref.log_row(a), ref.bar_b(a)
    assert np.isfinite(row).all()  # the NaN rows at t >= t_exec enter no sum
    for i, name in enumerate(ref.NAMES):
        if name in ref.COPIED:
            assert row[i] == want[name], name
        else:
            assert abs(row[i] - want[name]) <= bar[i], (name, row[i], want[name], bar[i])


def test_names_and_slots_are_the_models():
    """The restated constants against the package's (no device needed to read
    them from the sources)."""
    import ast
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "mog-asr_amd", "mog_air")
    src = open(os.path.join(pkg, "asr_model.py")).read()
    tree = ast.parse(src)
    qnames = None
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "Q":
            strings = [n.value for n in ast.walk(node.value)
                       if isinstance(n, ast.Constant) and isinstance(n.value, str)]
            qnames = "".join(strings).split()
    assert qnames is not None and len(qnames) == ref.NQ
    for name, slot in zip(("z_pres_kl", "scale_kl", "shift_kl", "pr_num"),
                          ("zkl", "skl", "shkl", "prn")):
        assert qnames.index(slot) == ref.SLOTS[name]
    ops_src = open(os.path.join(pkg, "ops.py")).read()
    for node in ast.walk(ast.parse(ops_src)):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "ASR_LOG_NAMES":
            assert tuple(ast.literal_eval(node.value)) == ref.NAMES
            break
    else:
        raise AssertionError("ops.ASR_LOG_NAMES not found")
