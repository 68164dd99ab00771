"""--summaries 1 of both entry points, called in process as
tests/test_gpu_graph_entry.py calls them: 12 iterations at batch 64 with the
cadence 4,8,8,4 (numeric, variables, images, gradients), under the eager and
the captured step.  The event file parses; the events sit at the reference's
steps with the reference's tags; the step-1 gradient summaries of the two graph
modes are equal; total_loss_all_dig at step 0 is the mean of per_image_loss of
the state saved at step 0 under the same test-model noise offsets."""
import glob
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
COMMON = ["-dn", "13", "--iterations", "12", "--batch-size", "64", "--synth-per-count", "40",
          "--no-images"]
SUMM = ["--summaries", "1", "--summary-cadence", "4,8,8,4"]
ASR = ["-gm", "100", "-gne", "10"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _run(entry_name, folder, key, extra, monkeypatch):
    entry = __import__(entry_name)
    monkeypatch.chdir(folder)
    step = entry.main(COMMON + ["-r", str(folder / "res"), "-k", key] + extra)
    assert step == 12
    return folder / ("res_(%s)" % key)


def _events(res):
    """[(step, {tag: (kind, payload)})] of the run's one event file, the
    file-version record checked and dropped."""
    from mog_air import records
    files = glob.glob(str(res / "summary" / "events.out.tfevents.*"))
    assert len(files) == 1, files
    recs = list(records.iter_records(files[0], verify=True))
    first = {fn: v for fn, _, v in records._fields(recs[0])}
    assert first[3] == b"brain.Event:2"
    out = []
    for rec in recs[1:]:
        ev = {fn: v for fn, _, v in records._fields(rec)}
        values = {}
        for fn, _, v in records._fields(ev[5]):
            assert fn == 1
            val = {f: x for f, _, x in records._fields(v)}
            tag = val[1].decode()
            assert tag not in values
            kind = {2: "scalar", 4: "image", 5: "histo"}[[f for f in val if f != 1][0]]
            values[tag] = (kind, val[[f for f in val if f != 1][0]])
        out.append((ev.get(2, 0), values))
    return out


def _kinds(events):
    """step -> the kinds of event at it: numeric / variables / images / gradients."""
    out = {}
    for step, values in events:
        tags = list(values)
        if any(t.endswith("_grad_applied") for t in tags):
            kind = "gradients"
        elif tags[0].startswith("reconstruction/image/"):
            kind = "images"
        elif values[tags[0]][0] == "histo":
            kind = "variables"
        else:
            kind = "numeric"
        out.setdefault(kind, []).append(step)
    return out


def _check_histo(payload):
    from mog_air import records
    h = {fn: v for fn, _, v in records._fields(payload)}
    lim, bkt = np.frombuffer(h[6], "<f8"), np.frombuffer(h[7], "<f8")
    assert len(lim) == len(bkt) and np.all(np.diff(lim) > 0)
    assert bkt.sum() == struct.unpack("<d", h[3])[0] > 0


def test_air_summaries_under_both_graph_modes(tmp_path, monkeypatch):
    from mog_air import checkpoint, summaries, trainer
    seen = {}
    real_pair, real_numeric = trainer.model_pair, summaries.Summaries.numeric

    def pair(*a, **k):
        seen["models"] = real_pair(*a, **k)
        return seen["models"]

    def numeric(self, test_model, images, digits, batch, step):
        if step == 0:
            seen["ctr"], seen["test"] = test_model._noise_ctr, (images, digits)
        return real_numeric(self, test_model, images, digits, batch, step)
    monkeypatch.setattr(trainer, "model_pair", pair)
    monkeypatch.setattr(summaries.Summaries, "numeric", numeric)

    by_mode = {}
    for graph in ("0", "1"):
        res = _run("training_air_original", tmp_path, "g" + graph, SUMM + ["--graph", graph],
                   monkeypatch)
        events = by_mode[graph] = _events(res)
        kinds = _kinds(events)
        assert kinds == {"numeric": [0, 4, 8], "variables": [0, 8], "images": [0, 8],
                         "gradients": [1, 5, 9]}, kinds
        train_model, test_model = seen["models"]
        names = [n for n, _ in train_model.params.specs]
        for step, values in events:
            tags = list(values)
            if step in (1, 5, 9):
                assert sorted(tags) == sorted(
                    [n + s for n in names
                     for s in ("_grad_applied", "_grad_applied_norm", "_grad_applied_avg")])
                for n in names:
                    assert values[n + "_grad_applied"][0] == "histo"
                    _check_histo(values[n + "_grad_applied"][1])
                    norm = struct.unpack("<f", values[n + "_grad_applied_norm"][1])[0]
                    assert 0.0 <= norm <= 1.0 + 1e-6  # clip_by_norm(1.0)
            elif tags[0].startswith("reconstruction/image/"):
                n_test = len(seen["test"][1])
                assert tags == ["reconstruction/image/%d" % i for i in range(min(60, n_test))]
                assert all(v[0] == "image" for v in values.values())
            elif values[tags[0]][0] == "histo":
                # a zero bias has values (all in one bucket), so every variable is there
                assert tags == names
                for v in values.values():
                    _check_histo(v[1])
            else:
                assert tags == summaries.numeric_tags(6, 6) and len(tags) == 320

        # total_loss_all_dig at step 0 against the state saved at step 0
        numeric0 = [v for s, v in events if s == 0 and "total_loss_all_dig" in v][0]
        got = struct.unpack("<f", numeric0["total_loss_all_dig"][1])[0]
        checkpoint.load_state(str(res / "models" / "air-state-0.npz"), train_model, test_model,
                              feed=None, ctx=trainer.Dist(), mode="resume")
        test_model._noise_ctr = seen["ctr"]
        images, digits = seen["test"]
        test_model.infer(images, digits)
        want = np.float32(test_model.per_image_loss.cpu().numpy().astype(np.float64).mean())
        print("graph", graph, "total_loss_all_dig", got, want)
        assert abs(np.float32(got) - want) <= np.spacing(np.abs(want))

    # same seeds, bit-identical steps: the two modes' gradient summaries at step 1
    g0 = [v for s, v in by_mode["0"] if s == 1][0]
    g1 = [v for s, v in by_mode["1"] if s == 1][0]
    assert g0 == g1


def test_asr_summaries_variables_and_gradients_only(tmp_path, monkeypatch):
    from mog_air import trainer
    seen = {}
    real_pair = trainer.model_pair

    def pair(*a, **k):
        seen["models"] = real_pair(*a, **k)
        return seen["models"]
    monkeypatch.setattr(trainer, "model_pair", pair)
    for graph in ("0", "1"):
        res = _run("train_air_pr", tmp_path, "g" + graph, ASR + SUMM + ["--graph", graph],
                   monkeypatch)
        events = _events(res)
        assert _kinds(events) == {"variables": [0, 8], "gradients": [1, 5, 9]}
        names = [n for n, _ in seen["models"][0].params.specs]
        for step, values in events:
            if step in (0, 8):
                assert list(values) == names
            else:
                assert len(values) == 3 * len(names)
                assert all((n + "_grad_applied") in values for n in names)


def test_summaries_0_writes_no_event_file(tmp_path, monkeypatch):
    res = _run("training_air_original", tmp_path, "off", ["--graph", "1"], monkeypatch)
    assert (res / "summary").is_dir()
    assert not glob.glob(str(res / "summary" / "events*"))
