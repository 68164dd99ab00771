"""The detection metrics on the device (csrc/eval_det.hip, ops.eval_detection,
evaluation.DeviceEvaluator) against the reference's own outputs
(tests/golden/eval_detection.npz) and against the host ``evaluation``.

Bars (tests/eval_device_cases.py check_against): precision / recall columns
0-21 of every image bit-equal; the three IoU columns within 2^-46 (two orders
of at most 8 addends in [0, 1]); the batch means within N 2^-52 + 2^-46 (numpy
sums sequentially over axis 0 and pairwise for the 1-D means, the kernel in
32 row segments).  The largest deviations are printed."""
import os

import numpy as np
import pytest
import torch

import eval_device_cases as edc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_detection.npz")
DEV = "cuda:0"


def _unflat(a, off):
    return [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as f:
        return dict(f)


@pytest.fixture(scope="module")
def case():
    return edc.random_case()


@pytest.fixture(scope="module")
def case_rows(case):
    """The host's per-image rows and means of the random case (computed once)."""
    return edc.host_per_image(*case), edc.host_means(*case)


def _run(pos, box, shifts, scales, num, chunks=None, csize=50):
    from mog_air.evaluation import DeviceEvaluator
    ev = DeviceEvaluator(pos, box, csize, DEV)
    n = len(pos)
    s = 0
    for c in chunks or [n]:
        ev.update(s, shifts[s:s + c], scales[s:s + c], num[s:s + c])
        s += c
    assert s == n
    return ev.per_image().cpu().numpy(), ev.means().cpu().numpy(), ev


@pytest.mark.parametrize("name", ["random", "edges", "hungary"])
def test_fixture_cases_float64(gold, name):
    pos = _unflat(gold[f"{name}_pos"], gold[f"{name}_pos_off"])
    box = _unflat(gold[f"{name}_box"], gold[f"{name}_box_off"])
    sh = torch.from_numpy(gold[f"{name}_shifts"]).to(DEV)
    sc = torch.from_numpy(gold[f"{name}_scales"]).to(DEV)
    assert sh.dtype == torch.float64
    num = torch.from_numpy(gold[f"{name}_num"].astype(np.int32)).to(DEV)
    per, means, ev = _run(pos, box, sh, sc, num)
    ref_means = np.concatenate([gold[f"{name}_precision"], gold[f"{name}_recall"],
                                gold[f"{name}_means"]])
    edc.check_against(per, means, gold[f"{name}_per_image"], ref_means, f"fixture {name}")
    p, r, gi, di, gl = ev.result()
    np.testing.assert_array_equal(np.concatenate([p, r, [gi, di, gl]]), means)


def _step_major(case):
    """The case as the models hold it: fp32 step-major buffers, read through
    the transposed views Results.rec_shifts / rec_scales return."""
    _, _, shifts, scales, num = case
    sh = torch.from_numpy(shifts.astype(np.float32).transpose(1, 0, 2).copy()).to(DEV)  # [T,N,2]
    sc = torch.from_numpy(scales[:, :, 0].astype(np.float32).T.copy()).to(DEV)          # [T,N]
    return sh, sc, torch.from_numpy(num).to(DEV)


def test_model_layout_fp32_views(case, case_rows):
    pos, box = case[0], case[1]
    sh, sc, num = _step_major(case)
    v_sh, v_sc = sh.transpose(0, 1), sc.transpose(0, 1).unsqueeze(-1)
    assert not v_sh.is_contiguous() and v_sh.data_ptr() == sh.data_ptr()
    per, means, _ = _run(pos, box, v_sh, v_sc, num)
    edc.check_against(per, means, *case_rows, "model layout, 8 steps")


def test_model_layout_fewer_steps_than_detections(case):
    """steps < T: the views end after 5 executed steps; detections 5..7 read
    as zero rows, which is what run_test's zero padding hands the host."""
    pos, box, shifts, scales, num_h = case
    sh, sc, num = _step_major(case)
    steps = 5
    v_sh, v_sc = sh[:steps].transpose(0, 1), sc[:steps].transpose(0, 1).unsqueeze(-1)
    per, means, _ = _run(pos, box, v_sh, v_sc, num)
    hs, hc = np.zeros_like(shifts), np.zeros_like(scales)
    hs[:, :steps], hc[:, :steps] = v_sh.cpu().numpy(), v_sc.cpu().numpy()
    edc.check_against(per, means, edc.host_per_image(pos, box, hs, hc, num_h),
                      edc.host_means(pos, box, hs, hc, num_h), "model layout, 5 of 8 steps")


def test_chunks_and_reruns_are_bit_identical(case):
    pos, box = case[0], case[1]
    sh, sc, num = _step_major(case)
    v_sh, v_sc = sh.transpose(0, 1), sc.transpose(0, 1).unsqueeze(-1)
    one, m_one, _ = _run(pos, box, v_sh, v_sc, num)
    parts, m_parts, _ = _run(pos, box, v_sh, v_sc, num, chunks=[100, 150, 50])
    again, m_again, _ = _run(pos, box, v_sh, v_sc, num)
    for a, b in ((one, parts), (one, again), (m_one, m_parts), (m_one, m_again)):
        assert a.tobytes() == b.tobytes()


def test_refusals(case):
    from mog_air import ops
    from mog_air.evaluation import THRESHOLDS, DeviceEvaluator
    nine = [np.arange(18, dtype=np.int32)]
    with pytest.raises(ValueError):
        DeviceEvaluator(nine, nine, 50, DEV)                       # G = 9
    ev = DeviceEvaluator([np.zeros(2, np.int32)], [np.ones(2, np.int32)], 50, DEV)
    num = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ev.update(0, torch.zeros(1, 9, 2, device=DEV), torch.zeros(1, 9, 1, device=DEV), num)  # T = 9
    with pytest.raises(ValueError):
        ev.update(0, torch.zeros(1, 3, 2), torch.zeros(1, 3, 1), num)  # CPU detections
    thr = torch.from_numpy(THRESHOLDS.copy())
    per = torch.zeros(1, 25, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.eval_detection(torch.zeros(1, 1, 4, dtype=torch.float64), torch.ones(1, dtype=torch.int32),
                           torch.zeros(1, 3, 2), torch.zeros(1, 3), num.cpu(), 50, thr, per)
    with pytest.raises(ValueError):
        ops.eval_detection_means(per, torch.zeros(25, dtype=torch.float64))
    with pytest.raises(ValueError):  # a chunk past the end of the test set
        ev.update(1, torch.zeros(1, 3, 2, device=DEV), torch.zeros(1, 3, 1, device=DEV), num)
    with pytest.raises(ValueError):  # shifts and scales of different dtypes
        ev.update(0, torch.zeros(1, 3, 2, device=DEV, dtype=torch.float64),
                  torch.zeros(1, 3, 1, device=DEV), num)
