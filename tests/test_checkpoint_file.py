"""mog_air.checkpoint's file-level functions on plain dicts (no model, no
device): the atomic write, latest(), the rotation and the variable checks."""
import os

import numpy as np
import pytest

from mog_air import checkpoint as ck

SPECS = [("air/rnn/a/weights", (3, 2)), ("air/rnn/a/biases", (2,))]


def _arrays(moments=True, seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in SPECS:
        for prefix in ("", "adam_m__", "adam_v__") if moments else ("",):
            out[prefix + ck.key_of(name)] = rng.standard_normal(shape).astype(np.float32)
    return out


def test_write_then_read_round_trips_without_pickle(tmp_path):
    arrays = _arrays()
    arrays["feed_buf"] = np.arange(5, dtype=np.int64)
    meta = {"format": ck.FORMAT_VERSION, "global_step": 7, "big": str(2 ** 100),
            "loop": {"rows": [[0.1, float("inf"), 3.0]]}}
    path = ck.write_file(ck.state_path(str(tmp_path), 7), arrays, meta)
    assert os.path.basename(path) == "air-state-7.npz"
    got, got_meta = ck.read_file(path)
    assert got_meta == meta and sorted(got) == sorted(arrays)
    for k in arrays:
        assert got[k].dtype == arrays[k].dtype
        np.testing.assert_array_equal(got[k], arrays[k])
    with np.load(path, allow_pickle=False) as z:  # nothing in it needs pickle
        assert "meta" in z.files and z["meta"].dtype.kind == "U"
    assert sorted(os.listdir(tmp_path)) == ["air-state-7.npz"]  # no temporary left behind


def test_a_variables_file_reads_as_arrays_without_meta(tmp_path):
    path = str(tmp_path / "air-model-0.npz")
    np.savez(path, **_arrays(moments=False))
    got, meta = ck.read_file(path)
    assert meta is None and sorted(got) == sorted(_arrays(moments=False))


def test_another_format_version_is_refused(tmp_path):
    path = ck.write_file(ck.state_path(str(tmp_path), 1), _arrays(), {"format": 99})
    with pytest.raises(ValueError, match="format 99"):
        ck.read_file(path)


def test_latest_ignores_leftover_temporaries_and_other_files(tmp_path):
    folder = str(tmp_path)
    assert ck.latest(folder) is None
    for step in (0, 10, 9):
        ck.write_file(ck.state_path(folder, step), _arrays(), {"format": ck.FORMAT_VERSION})
    # what a killed save leaves, and files that are no state files
    for name in ("air-state-20.npz.tmp-4242", "air-state-30.npz.tmp", "air-model-40.npz",
                 "air-state-final.npz", "air-state-50.npz.bak"):
        (tmp_path / name).write_bytes(b"truncated")
    assert ck.latest(folder) == ck.state_path(folder, 10)  # by step, not by name or age
    assert ck.resolve(folder) == ck.state_path(folder, 10)
    assert ck.resolve(ck.state_path(folder, 9)) == ck.state_path(folder, 9)
    with pytest.raises(ValueError, match="no such state file"):
        ck.resolve(ck.state_path(folder, 77))
    with pytest.raises(ValueError, match="no air-state"):
        empty = tmp_path / "empty"
        empty.mkdir()
        ck.resolve(str(empty))


def test_a_failed_write_leaves_the_old_file_and_no_temporary(tmp_path):
    folder = str(tmp_path)
    path = ck.write_file(ck.state_path(folder, 3), _arrays(seed=1), {"format": ck.FORMAT_VERSION})
    before = open(path, "rb").read()

    class Unserialisable:
        pass
    with pytest.raises(TypeError):
        ck.write_file(path, _arrays(seed=2), {"format": ck.FORMAT_VERSION,
                                              "x": Unserialisable()})
    with pytest.raises(ValueError):  # an object array needs pickle: np.savez refuses
        ck.write_file(path, {"bad": np.array([Unserialisable()], dtype=object)}, None)
    assert open(path, "rb").read() == before
    assert os.listdir(folder) == ["air-state-3.npz"]


def test_rotation_keeps_the_three_highest_steps(tmp_path):
    folder = str(tmp_path)
    (tmp_path / "air-model-0.npz").write_bytes(b"not mine")
    for step in (0, 10, 20, 30, 40):
        ck.write_file(ck.state_path(folder, step), _arrays(), {"format": ck.FORMAT_VERSION})
        ck.rotate(folder)
        kept = sorted(int(f.split("-")[2].split(".")[0]) for f in os.listdir(folder)
                      if f.startswith("air-state-"))
        assert kept == [s for s in (0, 10, 20, 30, 40) if s <= step][-3:]
    assert os.path.exists(tmp_path / "air-model-0.npz")
    assert ck.KEEP == 3


def test_state_files_do_not_match_the_variables_glob(tmp_path):
    import fnmatch
    assert not fnmatch.fnmatch(os.path.basename(ck.state_path("m", 5)), "air-model-*.npz")


def test_missing_variable_is_named():
    arrays = _arrays()
    del arrays["air__rnn__a__biases"]
    with pytest.raises(ValueError, match="air/rnn/a/biases"):
        ck.check_variables(SPECS, arrays, moments=True)


def test_missing_moment_is_named():
    arrays = _arrays()
    del arrays["adam_v__air__rnn__a__weights"]
    with pytest.raises(ValueError, match="adam_v__air__rnn__a__weights.*air/rnn/a/weights"):
        ck.check_variables(SPECS, arrays, moments=True)
    ck.check_variables(SPECS, arrays, moments=False)  # the variables alone are complete


def test_another_shape_is_named():
    arrays = _arrays()
    arrays["air__rnn__a__weights"] = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match=r"air/rnn/a/weights with shape \(2, 3\).*\(3, 2\)"):
        ck.check_variables(SPECS, arrays, moments=True)


def test_a_variable_the_model_lacks_is_named():
    arrays = _arrays()
    arrays["air__cnn__conv1__kernel"] = np.zeros((5, 5, 1, 8), np.float32)
    with pytest.raises(ValueError, match="air/cnn/conv1/kernel"):
        ck.check_variables(SPECS, arrays, moments=True)
    arrays.pop("air__cnn__conv1__kernel")
    arrays["feed_buf"] = np.zeros(3, np.int64)  # the file's own entries are no variables
    ck.check_variables(SPECS, arrays, moments=True)


def test_fp32_bit_patterns_round_trip():
    for v in (np.float32(0.9) ** 7, np.float32(0.999) ** 1234, np.float32(1e-40), np.float32(0)):
        bits = ck._f32_bits(v)
        assert isinstance(bits, int)
        back = ck._bits_f32(bits)
        assert back.dtype == np.float32 and back.tobytes() == np.float32(v).tobytes()
