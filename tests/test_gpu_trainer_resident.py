"""The trainers' --resident switch: run_test with a DeviceEvaluator against
run_test + the host evaluation, and both entry points run with --resident 0
and --resident 1 (same batches, same losses, same metrics)."""
import glob
import logging
import re
import types

import numpy as np
import pytest
import torch

import eval_device_cases as edc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _test_model(scope):
    from mog_air.air_model import AIRModel
    return AIRModel(max_steps=3, scale_prior_variance=0.05, z_pres_prior_log_odds=-0.01,
                    learning_rate=1e-4, gradient_clipping_norm=1.0, cnn=False, train=False,
                    scope=scope, device=DEV, seed=21, noise_seed=22)


def test_run_test_both_ways():
    """Two test models of one seed and one noise seed (the Philox offsets
    advance per call, so one model cannot serve both runs); 120 synthetic
    images in chunks of 50, 50 and 20."""
    from mog_air import trainer
    from mog_air.evaluation import evaluation
    args = types.SimpleNamespace(synth_per_count=300, data="mnist", dig_surfix="",
                                 write_synthetic=0, device=DEV, resident=1)
    log = logging.getLogger("test_resident")
    tr_x, _, test = trainer.load_data(args, "absent/a.tfrecords", "absent/b.tfrecords", [1, 3], log)
    assert len(test[1]) == 120
    host_model, dev_model = _test_model("resident_h"), _test_model("resident_d")
    tl, ta, tm, sc, sh, nd = trainer.run_test(host_model, test, 50, 50)
    assert trainer.resident_ok(args, tr_x, test, dev_model, log)
    test_dev, evaluator = trainer.resident_test_set(args, test, 50, dev_model)
    assert test_dev[0].is_cuda and test_dev[1].dtype == torch.int32
    dl, da, dm, ev = trainer.run_test(dev_model, test_dev, 50, 50, evaluator)
    assert ev is evaluator
    assert (dl, da, dm) == (tl, ta, tm)
    assert nd.sum() > 0  # the models do detect something: the metrics are not the special cases
    ref_rows = edc.host_per_image(test[3], test[4], sh, sc, nd)
    p, r, gi, di, gl = evaluation(test[3], test[4], sh, sc, nd, csize=50)
    ref_means = np.concatenate([p, r, [gi, di, gl]])
    edc.check_against(ev.per_image().cpu().numpy(), ev.means().cpu().numpy(), ref_rows,
                      ref_means, "run_test, 120 images")
    got = ev.result()
    assert got[0].shape == (11,) and got[1].shape == (11,) and isinstance(got[4], float)


def test_resident_falls_back_above_the_caps(caplog):
    from mog_air import trainer
    args = types.SimpleNamespace(device=DEV, resident=1)
    log = logging.getLogger("test_resident_caps")
    tr_x = np.zeros((4, 2500), np.float32)
    test = (np.zeros((2, 2500), np.float32), np.zeros(2, np.int32), None,
            [np.zeros(18, np.int32), np.zeros(2, np.int32)])
    model = types.SimpleNamespace(max_steps=3)
    with caplog.at_level(logging.WARNING, logger=log.name):
        assert not trainer.resident_ok(args, tr_x, test, model, log)          # 9 boxes
        ok = (test[0], test[1], None, [np.zeros(4, np.int32)] * 2)
        assert not trainer.resident_ok(args, tr_x, ok, types.SimpleNamespace(max_steps=9), log)
        assert trainer.resident_ok(args, tr_x, ok, model, log)
    assert len([r for r in caplog.records if "--resident 1 not taken" in r.getMessage()]) == 2
    args.resident = 0
    assert not trainer.resident_ok(args, tr_x, ok, model, log)


_FLOAT = re.compile(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?")


def _lines(folder):
    text = open(glob.glob(str(folder / "logfile*.log"))[0]).read()
    msgs = [ln.split("|", 1)[1] for ln in text.splitlines() if "|" in ln]
    losses = [m for m in msgs if "train loss" in m or "test loss" in m or m.startswith("step:")
              or ("TotLoss" in m and m.startswith("test:"))]
    metrics = [m for m in msgs if m.startswith("test:") and "precision:[" in m]
    # a numpy array printed over several lines continues without the '|' prefix
    blocks, cur = [], None
    for ln in text.splitlines():
        if "|" in ln:
            if cur is not None:
                blocks.append(cur)
            msg = ln.split("|", 1)[1]
            cur = msg if msg.startswith("test:") and "precision:[" in msg else None
        elif cur is not None:
            cur += " " + ln
    if cur is not None:
        blocks.append(cur)
    floats = [[float(v) for v in _FLOAT.findall(b.split("precision:", 1)[1])] for b in blocks]
    return losses, metrics, floats


def _both(entry, flags, tmp_path, key):
    out = []
    for resident in (0, 1):
        step = entry.main(flags + ["-r", str(tmp_path / f"res{resident}"), "-k", key,
                                   "--iterations", "21", "--synth-per-count", "40",
                                   "--resident", str(resident)])
        assert step == 21
        out.append(_lines(tmp_path / f"res{resident}_({key})"))
    (l0, m0, f0), (l1, m1, f1) = out
    assert l0 and l0 == l1, (l0, l1)
    assert m0 and len(m0) == len(m1) and len(f0) == len(f1) == len(m0)
    for a, b in zip(f0, f1):
        assert len(a) == len(b) >= 25
        assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-7, (a, b)


@pytest.mark.parametrize("flags", [["-dn", "13", "-data", "mnist"],
                                   ["-dn", "13", "-data", "mnist", "--cnn", "1"]])
def test_training_air_original_resident(tmp_path, monkeypatch, flags):
    import training_air_original as entry
    monkeypatch.chdir(tmp_path)
    _both(entry, flags, tmp_path, "t")


def test_train_air_pr_resident(tmp_path, monkeypatch):
    import train_air_pr as entry
    monkeypatch.chdir(tmp_path)
    _both(entry, ["-dn", "13", "-gm", "100", "-gne", "10"], tmp_path, "p")
