"""The train state under data parallelism: two gloo ranks on one device
(tests/gpu_ckpt_dp_worker.py, launched as tests/test_gpu_dp.py launches its
worker).  One launch takes steps with parallel.attach and saves; a second
launch loads into fresh models.  Each rank recovers its own noise seed and
counters (unequal shards advance them differently), a re-saved file equals
the original, and a file of two ranks is refused by a single process.

No bitwise claim on later steps: below WGRAD_TN_MIN_ROWS the data-parallel
weight gradients are atomic sums."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ckpt_cases as cc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(folder, phase):
    port = _free_port()
    procs = []
    for r in range(WORLD):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r),
                   WORLD_SIZE=str(WORLD), LOCAL_RANK="0", OMP_NUM_THREADS="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "gpu_ckpt_dp_worker.py"),
                                       folder, phase], env=env))
    try:
        rcs = [p.wait(timeout=100) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * WORLD
    return [dict(np.load(os.path.join(folder, f"{phase}_{r}.npz"))) for r in range(WORLD)]


def test_world2_save_and_load(tmp_path):
    from mog_air import checkpoint
    folder = str(tmp_path)
    os.mkdir(tmp_path / "again")
    saved = _launch(folder, "save")
    path = checkpoint.state_path(folder, 2)
    _, meta = checkpoint.read_file(path)
    assert meta["world"] == WORLD and len(meta["noise"]) == WORLD
    for r, s in enumerate(saved):
        assert meta["noise"][r] == {"train": [int(s["seeds"][0]), int(s["ctrs"][0])],
                                    "test": [int(s["seeds"][1]), int(s["ctrs"][1])]}
    # the shards (5 and 4 images) and the test batches (2 and 3) differ in size
    assert saved[0]["seeds"][0] != saved[1]["seeds"][0]
    assert saved[0]["ctrs"][0] != saved[1]["ctrs"][0] and saved[0]["ctrs"][1] != saved[1]["ctrs"][1]
    np.testing.assert_array_equal(saved[0]["crc"], saved[1]["crc"])  # one set of variables

    loaded = _launch(folder, "load")
    for s, ld in zip(saved, loaded):
        for k in ("seeds", "ctrs", "step", "crc", "next_picks"):
            np.testing.assert_array_equal(s[k], ld[k], err_msg=k)
    (a, am), (b, bm) = checkpoint.read_file(path), checkpoint.read_file(
        checkpoint.state_path(os.path.join(folder, "again"), 2))
    assert am == bm and sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k

    # a single process refuses the file of two ranks, and stays as it was
    train, test = cc.air_pair("fp32", "ckdp_w1", noise_seed=int(saved[0]["seeds"][0]))
    before = cc.snapshot(train, test)
    with pytest.raises(ValueError, match="saved by 2 ranks, this run has 1"):
        checkpoint.load_state(path, train, test)
    cc.assert_same(cc.snapshot(train, test), before, "refused")
