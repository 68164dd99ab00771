"""The iteration loop's cadence at iteration 200 for both entry points, called
in process as tests/test_gpu_graph_entry.py calls them: 200 eager iterations
at the default batch of 64 over a 16-image test set reach ten log lines, the
one periodic test pass and the final one.  What differs between the two
trainers there is pinned: AIR updates and prints its best-so-far only after
the periodic test and tags the final one 'final'; AIR-ASR does both after
every test and tags the final one with the step."""
import glob
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
COMMON = ["--synth-per-count", "40", "--no-images", "--iterations", "200", "--save-every", "0"]
AIR = ["-dn", "13"]
ASR = ["-dn", "13", "-gm", "100", "-gne", "10"]
BEST = ("elbo", "accu", "mse", "iou")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _run(entry_name, flags, folder, monkeypatch):
    entry = __import__(entry_name)
    monkeypatch.chdir(folder)  # results/ and data/ paths are relative, as in the reference
    step = entry.main(flags + COMMON + ["-r", str(folder / "res"), "-k", "c"])
    assert step == 200
    res = folder / "res_(c)"
    text = open(glob.glob(str(res / "logfile*.log"))[0]).read()
    # one message per record: the metrics lines print arrays, which wrap
    return res, [m.rstrip("\n") for m in
                 re.split(r"^\d\d:\d\d:\d\d;[A-Z]+\|", text, flags=re.M)[1:]]


def _where(msgs, start, having=""):
    return [i for i, m in enumerate(msgs) if m.startswith(start) and having in m]


def _fields(line):
    """name -> text of the name:value fields of a tab-separated log line."""
    return dict(f.split(":", 1) for f in line.split("\t") if ":" in f)


def _best(line):
    """The payload of a 'Current Best: ' / 'Final Best: ' line as four floats."""
    fields = _fields(line.split(": ", 1)[1])
    assert tuple(fields) == BEST
    return [float(fields[n]) for n in BEST]


def _final_state(res):
    from mog_air import checkpoint
    assert sorted(os.listdir(res / "models")) == ["air-state-200.npz"]  # and no air-model-*
    _, meta = checkpoint.read_file(str(res / "models" / "air-state-200.npz"))
    loop = meta["loop"]
    assert loop["step"] == 200 and loop["rows"] == [] and loop["logged"] == {}
    assert loop["update_flag"] is False
    return loop


def test_air_cadence_at_200(tmp_path, monkeypatch):
    res, msgs = _run("training_air_original", AIR, tmp_path, monkeypatch)
    train = [m for m in msgs if "\ttrain loss " in m]
    assert [m.split("\t")[0] for m in train] == ["iteration %d" % n for n in range(20, 201, 20)]
    (t200,) = _where(msgs, "iteration 200\ttest loss")
    (tfinal,) = _where(msgs, "iteration final\ttest loss")
    (m200,) = _where(msgs, "test:   200\tprecision:", "globaliou:")
    (mfinal,) = _where(msgs, "test:final\tprecision:", "globaliou:")
    (cur,) = _where(msgs, "Current Best:")
    (fin,) = _where(msgs, "Final Best:")
    assert t200 < m200 < cur < tfinal < mfinal < fin
    best = _best(msgs[cur])
    test_loss = msgs[t200].split("test loss ")[1].split("\t")[0]
    assert "{:.3f}".format(best[0]) == test_loss
    assert _best(msgs[fin]) == best  # the final test does not touch best

    loop = _final_state(res)
    assert loop["best"] == best
    losses = [float(m.split("train loss ")[1].split("\t")[0]) for m in train]
    assert "{:.3f}".format(loop["min_loss"]) == "{:.3f}".format(min(losses))


def test_asr_cadence_at_200(tmp_path, monkeypatch):
    from mog_air import ops
    names = ops.ASR_LOG_NAMES
    res, msgs = _run("train_air_pr", ASR, tmp_path, monkeypatch)
    train = [m for m in msgs if m.startswith("step:")]
    assert [m.split("\t")[0] for m in train] == ["step:{:6d}".format(n)
                                                 for n in range(20, 201, 20)]
    for m in train:
        assert tuple(_fields(m.split("\t", 1)[1])) == names
    metrics = _where(msgs, "test:   200\tprecision:", "global_iou:")
    variables = _where(msgs, "test:   200\t" + names[0])
    current = _where(msgs, "Current Best:")
    (fin,) = _where(msgs, "Final Best:")
    # the periodic test and the final one, which is tagged with the step
    assert len(metrics) == len(variables) == len(current) == 2
    assert metrics[0] < variables[0] < current[0] < metrics[1] < variables[1] < current[1] < fin
    assert not _where(msgs, "test:final") and not _where(msgs, "iteration final")
    best = _best(msgs[current[0]])
    # update_flag is already cleared at the final test
    assert _best(msgs[current[1]]) == best and _best(msgs[fin]) == best
    assert "{:.4f}".format(best[0]) == _fields(msgs[variables[0]])["elbo"]
    assert "{:.4f}".format(best[3]) == _fields(msgs[metrics[0]])["global_iou"]
    _final_state(res)
