"""The random case of tests/eval_device_cases.py is not trivial: checked with
the host ``evaluation`` alone, so the GPU test on it cannot pass on empty or
hit-free images."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import eval_device_cases as edc
from mog_air.evaluation import detection_boxes, iou_matrix


@pytest.fixture(scope="module")
def case():
    return edc.random_case()


@pytest.fixture(scope="module")
def rows(case):
    return edc.host_per_image(*case)


def test_shape_of_the_case(case):
    pos, box, shifts, scales, num = case
    assert len(pos) == edc.N == 300 and edc.N % 16 != 0
    assert shifts.shape == (300, 8, 2) and scales.shape == (300, 8, 1)
    g = np.array([len(p) // 2 for p in pos])
    assert set(g) == set(range(9)) and set(num.tolist()) == set(range(9))
    assert np.array_equal(shifts, shifts.astype(np.float32).astype(np.float64))
    assert np.array_equal(scales, scales.astype(np.float32).astype(np.float64))


def test_a_quarter_of_the_images_hit_at_threshold_half(rows):
    assert (rows[:, 0] > 0).mean() >= 0.25
    # and hits spread over the thresholds: the strictest ones are not all equal
    assert len(np.unique(rows[:, :11].sum(0))) >= 6


def test_a_tenth_of_the_images_have_six_by_six_matrices(case):
    pos, _, _, _, num = case
    k = np.minimum([len(p) // 2 for p in pos], num)
    assert (k >= 6).mean() >= 0.10


def test_each_special_case_occurs(case, rows):
    pos, _, _, _, num = case
    g = np.array([len(p) // 2 for p in pos])
    both, no_gt, no_det = (g == 0) & (num == 0), (g == 0) & (num > 0), (g > 0) & (num == 0)
    assert both.any() and no_gt.any() and no_det.any()
    assert np.array_equal(rows[both][0], np.ones(25))
    assert np.array_equal(rows[no_gt][0], np.r_[np.zeros(11), np.ones(11), np.zeros(3)])
    assert np.array_equal(rows[no_det][0], np.zeros(25))


def test_row_greedy_pairing_falls_short_somewhere(case):
    pos, box, shifts, scales, num = case
    short = 0
    for i in range(edc.N):
        g, d = len(pos[i]) // 2, int(num[i])
        if min(g, d) < 2:
            continue
        xy = np.asarray(pos[i], np.float64).reshape(-1, 2)
        gt = np.concatenate([xy, xy + np.asarray(box[i], np.float64).reshape(-1, 2)], axis=1)
        iou = iou_matrix(gt, detection_boxes(shifts[i], scales[i], d, edc.CSIZE))
        used, greedy = set(), 0.0
        for row in iou:
            free = [j for j in range(d) if j not in used]
            if not free:
                break
            j = max(free, key=lambda j: row[j])
            used.add(j)
            greedy += row[j]
        r, c = linear_sum_assignment(-iou)
        short += iou[r, c].sum() > greedy + 1e-3
    assert short >= 1
