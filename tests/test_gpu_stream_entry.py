"""--stream 1 / --batch-size of both entry points, called in process as
tests/test_gpu_checkpoint_entry.py calls them: a streamed run trains and logs
the usual lines, four iterations equal two + --restore + two more bit for bit,
and --batch-size alone (no stream) trains from the resident dataset."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
COMMON = ["--synth-per-count", "40", "--no-images"]
STREAM = ["--stream", "1", "--batch-size", "256", "--save-every", "2"]
AIR = ["-dn", "13"]
ASR = ["-dn", "13", "-gm", "100", "-gne", "10"]


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


@pytest.mark.parametrize("entry,flags,final", [
    ("training_air_original", AIR, "iteration final\ttest loss"),
    ("train_air_pr", ASR, "test:     4\tprecision:")])
def test_streamed_run_and_its_restore(tmp_path, monkeypatch, entry, flags, final):
    from mog_air import checkpoint
    step, res_a = _run(entry, flags, tmp_path, "a", STREAM + ["--iterations", "4"], monkeypatch)
    assert step == 4
    msgs = _messages(res_a)
    assert any(m.startswith(final) for m in msgs)
    assert any("training has ended" in m for m in msgs)
    assert any("Final Best: elbo:" in m for m in msgs)
    _, meta = checkpoint.read_file(str(res_a / "models" / "air-state-4.npz"))
    assert meta["feed"] == {"kind": "stream", "next": 4 * 256}
    assert meta["fingerprint"]["stream_seed"] == 12345 and meta["fingerprint"]["glyphs"] == 512
    with np.load(res_a / "models" / "air-state-4.npz") as z:
        assert np.isfinite(np.concatenate([z[k].ravel() for k in z.files
                                           if z[k].dtype == np.float32])).all()

    step, res_b = _run(entry, flags, tmp_path, "b",
                       STREAM + ["--iterations", "4", "--restore",
                                 str(res_a / "models" / "air-state-2.npz")], monkeypatch)
    assert step == 4
    assert any(m.startswith("Restored ") and m.endswith("step 2") for m in _messages(res_b))
    for name in ("air-state-2.npz", "air-state-4.npz"):
        _assert_files_equal(res_a / "models" / name, res_b / "models" / name)
    assert [m for m in _messages(res_b) if m.startswith(final)] == \
        [m for m in msgs if m.startswith(final)]
    # another stream is another run
    with pytest.raises(ValueError, match="fingerprint|dataset"):
        _run(entry, flags, tmp_path, "c",
             STREAM + ["--iterations", "4", "--stream-seed", "7", "--restore",
                       str(res_a / "models" / "air-state-2.npz")], monkeypatch)


def test_stream_refusals_at_the_entry_point(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="needs --iterations"):
        _run("training_air_original", AIR, tmp_path, "n", ["--stream", "1"], monkeypatch)
    os.makedirs(tmp_path / "data" / "multi_mnist_data")
    open(tmp_path / "data" / "multi_mnist_data" / "test13.tfrecords", "wb").close()
    with pytest.raises(ValueError, match="exist"):
        _run("train_air_pr", ASR, tmp_path, "f", ["--stream", "1", "--iterations", "4"],
             monkeypatch)
    assert not glob.glob(str(tmp_path / "res*"))  # refused before anything is written


def test_batch_size_alone_trains_from_the_resident_set(tmp_path, monkeypatch):
    step, res = _run("training_air_original", AIR, tmp_path, "r",
                     ["--batch-size", "128", "--stream", "0", "--resident", "1",
                      "--synth-per-count", "200", "--iterations", "20"], monkeypatch)
    assert step == 20
    msgs = _messages(res)
    line = [m for m in msgs if m.startswith("iteration 20\ttrain loss")]
    assert len(line) == 1 and np.isfinite(float(line[0].split("train loss ")[1].split("\t")[0]))
    assert any(m.startswith("iteration final\ttest loss") for m in msgs)
    from mog_air import checkpoint
    _, meta = checkpoint.read_file(str(res / "models" / "air-state-20.npz"))
    assert meta["feed"]["index"] + meta["feed"]["epoch"] * meta["fingerprint"]["examples"] \
        >= 20 * 128  # 128 images per step left the dataset
