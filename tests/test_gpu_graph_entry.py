"""--graph 1 of both entry points, called in process as
tests/test_gpu_stream_entry.py calls them: 24 iterations at the default batch
of 64 with the captured step and the device log ring (run B) against the same
run with the eager step and its per-step host reads (run A), and against
--graph 1 --restore of A's state at step 10, in the middle of a 20-row block
(run C).

AIR: the three state files and the log lines are equal (the captured step is
the eager step bit for bit, the ring carries the means' bits).  AIR-ASR: every
array and the loop's decisions are equal; a logged value other than TotLoss /
accu / num_margin is a float64 device sum in B and C and an fp32 torch
reduction in A, so it is compared within bar (b) of tests/asr_log_row_ref.py,
with sum|x| taken from the train model's workspace at every push of run B."""
import glob

import numpy as np
import pytest
import torch

import asr_log_row_ref as ref

pytestmark = pytest.mark.gpu
COMMON = ["--synth-per-count", "40", "--no-images", "--iterations", "24", "--save-every", "10"]
AIR = ["-dn", "13"]
ASR = ["-dn", "13", "-gm", "100", "-gne", "10"]
STATES = ("air-state-10.npz", "air-state-20.npz", "air-state-24.npz")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _run(entry_name, flags, folder, key, extra, monkeypatch):
    entry = __import__(entry_name)
    monkeypatch.chdir(folder)  # results/ and data/ paths are relative, as in the reference
    step = entry.main(flags + COMMON + ["-r", str(folder / "res"), "-k", key] + extra)
    return step, folder / ("res_(%s)" % key)


def _messages(res):
    text = open(glob.glob(str(res / "logfile*.log"))[0]).read()
    return [ln.split("|", 1)[1] if "|" in ln else ln for ln in text.splitlines()]


def _assert_files_equal(a, b):
    from mog_air import checkpoint
    (aa, am), (ba, bm) = checkpoint.read_file(str(a)), checkpoint.read_file(str(b))
    assert am == bm, {k: (am[k], bm[k]) for k in am if am[k] != bm.get(k) and k != "specs"}
    assert sorted(aa) == sorted(ba)
    for k in aa:
        assert aa[k].dtype == ba[k].dtype and aa[k].tobytes() == ba[k].tobytes(), k


def _boom(*a, **k):
    raise AssertionError("a per-step host read under --graph 1")


def _count_drains(monkeypatch):
    from mog_air import trainer
    calls, real = [], trainer.LogRing.drain

    def drain(self):
        rows = real(self)
        calls.append(len(rows))
        return rows
    monkeypatch.setattr(trainer.LogRing, "drain", drain)
    return calls


# --------------------------------------------------------------------- AIR ---
def test_air_graph_run_equals_eager_run(tmp_path, monkeypatch):
    from mog_air import checkpoint
    from mog_air.model_base import ModelBase
    step, res_a = _run("training_air_original", AIR, tmp_path, "a", ["--graph", "0"], monkeypatch)
    assert step == 24
    with monkeypatch.context() as mp:
        mp.setattr(ModelBase, "step", _boom)
        drains = _count_drains(mp)
        step, res_b = _run("training_air_original", AIR, tmp_path, "b", ["--graph", "1"], mp)
    assert step == 24
    # one log line (20), four state saves (0, 10, 20, the final 24), the loop's end
    assert len(drains) in (6, 7) and sum(drains) == 24 and drains.count(0) >= 2, drains
    assert max(drains) == 10
    step, res_c = _run("training_air_original", AIR, tmp_path, "c",
                       ["--graph", "1", "--restore", str(res_a / "models" / "air-state-10.npz")],
                       monkeypatch)
    assert step == 24
    for name in STATES:
        _assert_files_equal(res_a / "models" / name, res_b / "models" / name)
    for name in STATES[1:]:
        _assert_files_equal(res_a / "models" / name, res_c / "models" / name)
    for name, pending in zip(STATES, (10, 0, 4)):
        _, meta = checkpoint.read_file(str(res_b / "models" / name))
        assert len(meta["loop"]["rows"]) == pending
    msgs = _messages(res_a)
    for start in ("iteration 20\ttrain loss", "iteration final\ttest loss"):
        line = [m for m in msgs if m.startswith(start)]
        assert len(line) == 1
        assert [m for m in _messages(res_b) if m.startswith(start)] == line
        assert [m for m in _messages(res_c) if m.startswith(start)] == line


# ----------------------------------------------------------------- AIR-ASR ---
def _asr_state_close(a, b, bars):
    """State files a (eager) and b (--graph 1): arrays byte-equal, meta equal
    but for loop.logged, which is equal for the copied entries and within bar
    (b) elsewhere; bars: step -> bar (b) per entry."""
    from mog_air import checkpoint
    (aa, am), (ba, bm) = checkpoint.read_file(str(a)), checkpoint.read_file(str(b))
    assert sorted(aa) == sorted(ba)
    for k in aa:
        assert aa[k].dtype == ba[k].dtype and aa[k].tobytes() == ba[k].tobytes(), k
    la, lb = dict(am["loop"]), dict(bm["loop"])
    ga, gb = la.pop("logged"), lb.pop("logged")
    assert la == lb  # step, min_loss, update_flag, best, rows
    assert {k: v for k, v in am.items() if k != "loop"} == \
        {k: v for k, v in bm.items() if k != "loop"}
    assert sorted(ga) == sorted(gb)
    first = am["loop"]["step"] - (len(ga["TotLoss"]) if ga else 0) + 1
    for i, name in enumerate(ref.NAMES if ga else ()):
        assert len(ga[name]) == len(gb[name])
        for j, (va, vb) in enumerate(zip(ga[name], gb[name])):
            print(a.name, name, first + j, repr(va), repr(vb), bars[first + j][i])
            if name in ref.COPIED:
                assert va == vb, (name, first + j)
            else:
                assert abs(va - vb) <= bars[first + j][i], (name, first + j, va, vb)
    return len(ga["TotLoss"]) if ga else 0


def _line_numbers(res, start):
    line = [m for m in _messages(res) if m.startswith(start)]
    assert len(line) == 1, line
    return {f.split(":")[0]: float(f.split(":")[1])
            for f in line[0].split("\t")[1:] if ":" in f}


def test_asr_graph_run_matches_eager_run(tmp_path, monkeypatch):
    from mog_air import trainer
    step, res_a = _run("train_air_pr", ASR, tmp_path, "a", ["--graph", "0"], monkeypatch)
    assert step == 24

    bars = {}  # train step -> bar (b) of its log row, from the workspace it was formed from
    real_push = trainer.LogRing.push

    def push(self, model):
        real_push(self, model)
        arrays = {k: getattr(model._ws, k).detach().cpu().numpy() for k in ref.ARRAYS}
        bars[model.global_step] = ref.bar_b(arrays)

    def guarded(self):
        if self.train:
            _boom()
        return real_lv.fget(self)

    from mog_air.asr_model import AIRModel as AsrModel
    from mog_air.model_base import ModelBase
    real_lv = AsrModel.__dict__["log_variables"]
    with monkeypatch.context() as mp:
        mp.setattr(ModelBase, "step", _boom)
        mp.setattr(AsrModel, "log_variables", property(guarded))  # the test model's stays usable
        mp.setattr(trainer.LogRing, "push", push)
        drains = _count_drains(mp)
        step, res_b = _run("train_air_pr", ASR, tmp_path, "b", ["--graph", "1"], mp)
    assert step == 24 and sorted(bars) == list(range(1, 25))
    assert len(drains) in (6, 7) and sum(drains) == 24, drains
    step, res_c = _run("train_air_pr", ASR, tmp_path, "c",
                       ["--graph", "1", "--restore", str(res_a / "models" / "air-state-10.npz")],
                       monkeypatch)
    assert step == 24

    for res, files in ((res_b, STATES), (res_c, STATES[1:])):
        pending = [_asr_state_close(res_a / "models" / n, res / "models" / n, bars)
                   for n in files]
        assert pending == [10, 0, 4][-len(files):]
    # the log line at step 20: the means of rows 1..20, printed with four decimals
    start = "step:    20\t"
    want = _line_numbers(res_a, start)
    assert tuple(want) == ref.NAMES
    line_bar = np.mean([bars[s] for s in range(1, 21)], axis=0) + 5e-5
    for res in (res_b, res_c):
        got = _line_numbers(res, start)
        for i, name in enumerate(ref.NAMES):
            print(res.name, name, got[name], want[name], line_bar[i])
            if name in ref.COPIED:
                assert got[name] == want[name], name
            else:
                assert abs(got[name] - want[name]) <= line_bar[i], (name, got[name], want[name])


# --------------------------------------------------------------- refusals ---
def test_graph_refusals(tmp_path, monkeypatch):
    import argparse

    from mog_air import trainer
    monkeypatch.chdir(tmp_path)
    parser = argparse.ArgumentParser()
    trainer.add_common_args(parser, reader_threads=1)
    assert parser.parse_args([]).graph == 0  # the default
    args = parser.parse_args(["--graph", "1", "-r", str(tmp_path / "res")])
    with pytest.raises(ValueError, match="single"):
        trainer.check_graph_args(args, trainer.Dist(0, 2))
    with pytest.raises(ValueError, match="single"):
        trainer.check_graph_args(args, trainer.Dist(1, 2), annealed=("z_pres_prior_log_odds",))
    with pytest.raises(ValueError, match="frozen"):
        trainer.check_graph_args(args, trainer.Dist(), annealed=("learning_rate",))
    trainer.check_graph_args(args, trainer.Dist(), annealed=("z_pres_prior_log_odds",))
    trainer.check_graph_args(parser.parse_args(["--graph", "0"]), trainer.Dist(0, 2))
    # at the entry point: a second rank's environment is refused before the
    # results folder (and before any process group) exists
    entry = __import__("training_air_original")

    def two_ranks(a):
        return trainer.Dist(0, 2)
    monkeypatch.setattr(trainer, "distributed_setup", two_ranks)
    with pytest.raises(ValueError, match="single"):
        entry.main(AIR + COMMON + ["--graph", "1", "-r", str(tmp_path / "res"), "-k", "x"])
    assert not glob.glob(str(tmp_path / "res*"))
