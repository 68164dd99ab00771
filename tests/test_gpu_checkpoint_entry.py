"""--restore / --save-every / --eval-only of both entry points, called in
process as tests/test_gpu_entry.py calls them (and once as a fresh process).

Run A trains 50 iterations and saves every 10; it keeps air-state-30 / 40 /
50 (the newest three; 50 is the state written before the final test).  Run B
continues A's air-state-30: 30 is no multiple of the 20-iteration log
cadence, so B's 'iteration 40' line needs the 10 rows saved with the state."""
import contextlib
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--synth-per-count", "40", "--no-images"]
AIR = ["-dn", "13"]
ASR = ["-dn", "13", "-gm", "100", "-gne", "10"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


@contextlib.contextmanager
def _cwd(path):
    """results/ and data/ paths are relative, as in the reference."""
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def _run(entry_name, flags, folder, key, extra):
    entry = __import__(entry_name)
    with _cwd(folder):
        step = entry.main(flags + COMMON + ["-r", str(folder / "res"), "-k", key] + extra)
    return step, folder / ("res_(%s)" % key)


def _messages(res):
    """The log without its timestamps: 'HH:MM:SS;LEVEL|message' -> message; a
    numpy array printed over several lines continues without the prefix."""
    text = open(glob.glob(str(res / "logfile*.log"))[0]).read()
    return [ln.split("|", 1)[1] if "|" in ln else ln for ln in text.splitlines()]


def _tail(res, start):
    """Every log line from the first that starts with ``start``."""
    msgs = _messages(res)
    first = [i for i, m in enumerate(msgs) if m.startswith(start)]
    assert first, (start, msgs[-12:])
    return msgs[first[0]:]


def _assert_files_equal(a, b):
    from mog_air import checkpoint
    (aa, am), (ba, bm) = checkpoint.read_file(str(a)), checkpoint.read_file(str(b))
    assert am == bm, {k: (am[k], bm[k]) for k in am if am[k] != bm.get(k) and k != "specs"}
    assert sorted(aa) == sorted(ba)
    for k in aa:
        assert aa[k].dtype == ba[k].dtype and aa[k].tobytes() == ba[k].tobytes(), k


def _states(res):
    return sorted(os.path.basename(p) for p in glob.glob(str(res / "models" / "air-state-*")))


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    folder = tmp_path_factory.mktemp("air_a")
    step, res = _run("training_air_original", AIR, folder, "a",
                     ["--iterations", "50", "--save-every", "10"])
    assert step == 50
    assert _states(res) == ["air-state-30.npz", "air-state-40.npz", "air-state-50.npz"]
    # the variables files are what they were: the newest three of 0 .. 40
    assert sorted(os.path.basename(p) for p in glob.glob(str(res / "models" / "air-model-*"))) \
        == ["air-model-20.npz", "air-model-30.npz", "air-model-40.npz"]
    with np.load(res / "models" / "air-model-40.npz") as z:
        assert all(k.startswith("air__") for k in z.files)
    return res


def test_resumed_run_equals_the_uninterrupted_one(run_a, tmp_path):
    step, res = _run("training_air_original", AIR, tmp_path, "b",
                     ["--restore", str(run_a / "models" / "air-state-30.npz"),
                      "--iterations", "50", "--save-every", "10"])
    assert step == 50
    assert res != run_a  # a resumed run writes into its own results folder
    assert any(m.startswith("Restored ") and "air-state-30.npz" in m and m.endswith("step 30")
               for m in _messages(res))
    assert _states(res) == ["air-state-30.npz", "air-state-40.npz", "air-state-50.npz"]
    for name in ("air-state-30.npz", "air-state-40.npz", "air-state-50.npz"):
        _assert_files_equal(run_a / "models" / name, res / "models" / name)
    tail_a, tail_b = _tail(run_a, "iteration 40\ttrain loss"), _tail(res, "iteration 40\ttrain loss")
    assert any(m.startswith("iteration final\ttest loss") for m in tail_a)
    assert any(m.startswith("test:final\tprecision:[") for m in tail_a)
    assert tail_b == tail_a
    assert not any(m.startswith("iteration 20\t") for m in _messages(res))


def test_resumed_run_as_a_fresh_process(run_a, tmp_path):
    """Module-level state that an in-process run inherits would hide a
    value the state file lacks: once as a process of its own."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "training_air_original.py")] + AIR + COMMON +
        ["-r", str(tmp_path / "res"), "-k", "s", "--restore",
         str(run_a / "models" / "air-state-30.npz"), "--restore-mode", "resume",
         "--eval-only", "0", "--iterations", "50", "--save-every", "10"],
        cwd=str(tmp_path), timeout=240, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = tmp_path / "res_(s)"
    for name in ("air-state-30.npz", "air-state-40.npz", "air-state-50.npz"):
        _assert_files_equal(run_a / "models" / name, res / "models" / name)
    assert _tail(res, "iteration 40\ttrain loss") == _tail(run_a, "iteration 40\ttrain loss")


def test_eval_only_repeats_the_final_test(run_a, tmp_path):
    step, res = _run("training_air_original", AIR, tmp_path, "c",
                     ["--restore", str(run_a / "models" / "air-state-50.npz"), "--eval-only", "1"])
    assert step == 50
    assert _tail(res, "iteration final\ttest loss") == _tail(run_a, "iteration final\ttest loss")
    assert not any("train loss" in m for m in _messages(res))
    assert _states(res) == []  # an evaluation saves nothing


def test_eval_only_needs_restore(tmp_path):
    with pytest.raises(ValueError, match="--eval-only 1 needs --restore"):
        _run("training_air_original", AIR, tmp_path, "e", ["--eval-only", "1"])


def test_restore_mode_weights_from_a_variables_file(run_a, tmp_path):
    from mog_air import model_base
    path = run_a / "models" / "air-model-40.npz"
    step, res = _run("training_air_original", AIR, tmp_path, "w",
                     ["--restore", str(path), "--restore-mode", "weights", "--eval-only", "1"])
    assert step == 0
    params = model_base._SCOPES["air"]
    assert params.global_step == 0 and params.adam_t == 0
    assert float(params.m.abs().max()) == 0.0
    got = params.state_dict()
    with np.load(path) as z:
        assert sorted(z.files) == sorted(k.replace("/", "__") for k in got)
        for k, v in got.items():
            assert v.tobytes() == z[k.replace("/", "__")].tobytes(), k
    # a variables file is no state to resume from
    with pytest.raises(ValueError, match="holds variables only"):
        _run("training_air_original", AIR, tmp_path, "w2",
             ["--restore", str(path), "--iterations", "1"])


def test_train_air_pr_save_restore_and_eval(tmp_path):
    step, res_a = _run("train_air_pr", ASR, tmp_path, "pa",
                       ["--iterations", "50", "--save-every", "10"])
    assert step == 50
    assert _states(res_a) == ["air-state-30.npz", "air-state-40.npz", "air-state-50.npz"]
    step, res_b = _run("train_air_pr", ASR, tmp_path, "pb",
                       ["--restore", str(res_a / "models" / "air-state-30.npz"),
                        "--iterations", "50", "--save-every", "10"])
    assert step == 50
    # the state written on arrival is the state that was read
    _assert_files_equal(res_a / "models" / "air-state-30.npz",
                        res_b / "models" / "air-state-30.npz")
    line = [m for m in _messages(res_b) if m.startswith("step:    40\t")]
    assert len(line) == 1
    names = [f.split(":")[0] for f in line[0].split("\t")[1:] if f]
    ref = [m for m in _messages(res_a) if m.startswith("step:    40\t")][0]
    assert names == [f.split(":")[0] for f in ref.split("\t")[1:] if f]  # the model's order
    tot = float([f for f in line[0].split("\t") if f.startswith("TotLoss:")][0].split(":")[1])
    assert np.isfinite(tot)
    assert any(m.startswith("training has ended") or m == "training has ended"
               for m in _messages(res_b))
    # the evaluation of each run's final state repeats that run's final test
    for key, res in (("pca", res_a), ("pcb", res_b)):
        step, res_c = _run("train_air_pr", ASR, tmp_path, key,
                           ["--restore", str(res / "models"), "--eval-only", "1"])
        assert step == 50
        assert _tail(res_c, "test:    50\tprecision:") == _tail(res, "test:    50\tprecision:")
