"""bench.py's command line: a plain run prints the headline line alone
(``ms_per_step`` over exactly ``--steps`` timed steps, none of the ``--full``
measurements) and ``--dump-outputs DIR`` writes the last timed step's outputs
as float32 ``DIR/<name>.npy``, at most 64 MB, the same from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "configs_1_bf16", "config_1_batch64_fp32", "fused_step_roofline",
             "fp32_step_roofline", "cpu_baseline")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _bench(out_dir, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--batch", "64", "--dump-outputs",
                        str(out_dir)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_a")
    line = _bench(d, 3)
    return line, {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(str(d / "*.npy")))}


def test_plain_run_line_and_dump(first_run):
    a, arrays = first_run
    assert a["steps"] == 3 and a["unit"] == "images/sec" and a["higher_is_better"] is True
    assert a["dtype"] == "fp32" and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(64 / (a["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in a]
    assert {"means", "per_image_loss", "rec_num_digits", "grads", "params"} <= set(arrays)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64e6
    assert arrays["per_image_loss"].shape == (64,)
    assert arrays["means"][0] == pytest.approx(a["config"]["loss_last"], rel=1e-6)


def test_dump_is_the_same_from_run_to_run(first_run, tmp_path):
    arrays = first_run[1]
    # the same arguments: the same inputs, so the same step up to the order of
    # the split-K atomic sums of the weight gradients (fp32 rounding, the
    # 1e-5 of tests/test_gpu_dp.py; the per-image records see it only through
    # the parameters of the earlier steps)
    _bench(tmp_path / "b", 3)
    for name, v in arrays.items():
        w = np.load(str(tmp_path / "b" / (name + ".npy")))
        assert w.shape == v.shape
        if name in ("grads", "params"):
            assert np.linalg.norm(w - v) <= 1e-5 * np.linalg.norm(v), name
        else:
            np.testing.assert_allclose(w, v, rtol=1e-5, atol=1e-6)
