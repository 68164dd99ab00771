"""Detection metrics of the inferred objects, restating
air/evaluation_detection.py:5-98 on the host: per image, the IoU matrix of
ground-truth boxes against the boxes implied by the inferred (scale, shift),
precision / recall at IoU thresholds 0.50, 0.55, ..., 1.00, the mean best IoU
per ground-truth box and per detection, and the Hungarian-matched global IoU
(scipy.optimize.linear_sum_assignment, as the reference).

Box conventions (evaluation_detection.py:5-25, :43-57): ground truth
[x1, y1, x1 + w, y1 + h] from (positions, boxes); a detection is the square
of half-side scale * C/2 centred at ((tx + 1) C/2, (ty + 1) C/2); IoU uses
the inclusive-pixel "+1" areas.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

THRESHOLDS = 0.5 + 0.05 * np.arange(11)


def iou_matrix(gt: np.ndarray, det: np.ndarray) -> np.ndarray:
    """IoU of every gt box [G, 4] against every detection [D, 4]
    (evaluation_detection.py:5-25, vectorised)."""
    xa = np.maximum(gt[:, None, 0], det[None, :, 0])
    ya = np.maximum(gt[:, None, 1], det[None, :, 1])
    xb = np.minimum(gt[:, None, 2], det[None, :, 2])
    yb = np.minimum(gt[:, None, 3], det[None, :, 3])
    inter = np.maximum(0, xb - xa + 1) * np.maximum(0, yb - ya + 1)
    area_g = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    area_d = (det[:, 2] - det[:, 0] + 1) * (det[:, 3] - det[:, 1] + 1)
    return inter / (area_g[:, None] + area_d[None, :] - inter).astype(np.float64)


def detection_boxes(shifts: np.ndarray, scales: np.ndarray, n: int, csize: int) -> np.ndarray:
    half = csize / 2
    cx = (shifts[:n, 0] + 1) * half
    cy = (shifts[:n, 1] + 1) * half
    r = scales[:n, 0] * half
    return np.stack([cx - r, cy - r, cx + r, cy + r], axis=1)


def evaluation(gt_position_xy, gt_scale_xy, inf_shifts, inf_scales, inf_num, csize=50):
    """(mean precision[11], mean recall[11], mean gt best-IoU, mean detection
    best-IoU, mean global IoU) over the images (evaluation_detection.py:28-98).
    inf_shifts [N, T, 2], inf_scales [N, T, 1], inf_num [N]."""
    inf_shifts = np.asarray(inf_shifts, np.float64)
    inf_scales = np.asarray(inf_scales, np.float64)
    n_img = len(gt_position_xy)
    precision = np.zeros((n_img, THRESHOLDS.size))
    recall = np.zeros((n_img, THRESHOLDS.size))
    gt_best = np.zeros(n_img)
    det_best = np.zeros(n_img)
    global_iou = np.zeros(n_img)
    for i in range(n_img):
        pos = np.asarray(gt_position_xy[i], np.float64)
        size = np.asarray(gt_scale_xy[i], np.float64)
        n_gt, n_det = len(pos) // 2, int(inf_num[i])
        if n_gt == 0 and n_det == 0:
            precision[i] = recall[i] = 1.0
            gt_best[i] = det_best[i] = global_iou[i] = 1.0
            continue
        if n_gt == 0:
            recall[i] = 1.0
            continue
        if n_det == 0:
            continue
        xy = pos.reshape(-1, 2)
        gt = np.concatenate([xy, xy + size.reshape(-1, 2)], axis=1)
        iou = iou_matrix(gt, detection_boxes(inf_shifts[i], inf_scales[i], n_det, csize))
        hit = (iou[None, :, :] > THRESHOLDS[:, None, None]).any(axis=1).sum(axis=1)
        precision[i] = hit / n_det
        recall[i] = hit / n_gt
        gt_best[i] = iou.max(axis=1).mean()
        det_best[i] = iou.max(axis=0).mean()
        r, c = linear_sum_assignment(-iou)
        global_iou[i] = iou[r, c].sum() / max(n_det, n_gt)
    return (precision.mean(0), recall.mean(0), gt_best.mean(), det_best.mean(),
            global_iou.mean())


EVAL_CAP = 8  # ground-truth boxes / loop steps per image of the device kernel (csrc/eval_det.hip)


def gt_box_table(gt_position_xy, gt_scale_xy):
    """(boxes [N, G, 4] float64 = [x, y, x + w, y + h], counts [N] int32) of
    the per-image lists, as ``evaluation`` builds each image's boxes (xy +
    size in float64, list order); G = the largest count (at least 1), unused
    slots zero."""
    n_img = len(gt_position_xy)
    num = np.asarray([len(p) // 2 for p in gt_position_xy], np.int32).reshape(n_img)
    G = max(1, int(num.max()) if n_img else 1)
    boxes = np.zeros((n_img, G, 4), np.float64)
    for i in range(n_img):
        g = int(num[i])
        if g:
            xy = np.asarray(gt_position_xy[i], np.float64)[:2 * g].reshape(-1, 2)
            size = np.asarray(gt_scale_xy[i], np.float64).reshape(-1, 2)
            boxes[i, :g] = np.concatenate([xy, xy + size], axis=1)
    return boxes, num


class DeviceEvaluator:
    """``evaluation`` on the device (ops.eval_detection): the ground-truth
    boxes are uploaded once; ``update`` takes each chunk's detections as
    device tensors (the test model's rec_shifts / rec_scales views are read in
    place) without a host synchronisation; ``result`` is the 5-tuple of
    ``evaluation`` after one 25-double copy.  At most EVAL_CAP boxes per image
    and EVAL_CAP loop steps (ValueError above either)."""

    def __init__(self, gt_position_xy, gt_scale_xy, csize, device, max_steps: int = EVAL_CAP):
        import torch

        from . import ops
        assert ops.EVAL_CAP == EVAL_CAP
        boxes, num = gt_box_table(gt_position_xy, gt_scale_xy)
        if boxes.shape[1] > EVAL_CAP:
            raise ValueError(f"{boxes.shape[1]} ground-truth boxes in one image: the device "
                             f"metrics hold {EVAL_CAP}")
        if not 0 <= max_steps <= EVAL_CAP:
            raise ValueError(f"max_steps {max_steps}: the device metrics hold {EVAL_CAP}")
        self._ops, self.csize, self.max_steps = ops, float(csize), int(max_steps)
        self.n_images = boxes.shape[0]
        self.gt_boxes = torch.from_numpy(boxes).to(device)
        self.gt_num = torch.from_numpy(num).to(device)
        self.thresholds = torch.from_numpy(np.ascontiguousarray(THRESHOLDS, np.float64)).to(device)
        self._per_image = torch.zeros((self.n_images, ops.EVAL_COLUMNS), dtype=torch.float64,
                                      device=device)
        self._means = torch.zeros(ops.EVAL_COLUMNS, dtype=torch.float64, device=device)

    def update(self, offset: int, rec_shifts, rec_scales, rec_num) -> None:
        """Images [offset, offset + n): rec_shifts [n, steps, 2], rec_scales
        [n, steps(, 1)] (fp32 or fp64, any strides), rec_num [n] int32."""
        if rec_shifts.dim() == 3 and rec_shifts.shape[1] > self.max_steps:
            raise ValueError(f"{rec_shifts.shape[1]} loop steps, the evaluator was built for "
                             f"{self.max_steps}")
        self._ops.eval_detection(self.gt_boxes, self.gt_num, rec_shifts, rec_scales, rec_num,
                                 self.csize, self.thresholds, self._per_image, offset=offset,
                                 max_steps=self.max_steps)

    def per_image(self):
        """[N, 25] float64 on the device: precision[11], recall[11], gt
        best-IoU, detection best-IoU, global IoU of every image."""
        return self._per_image

    def means(self):
        """The 25 batch means on the device (a fixed summation order)."""
        self._ops.eval_detection_means(self._per_image, self._means)
        return self._means

    def result(self):
        m = self.means().cpu().numpy()
        return m[:11].copy(), m[11:22].copy(), float(m[22]), float(m[23]), float(m[24])
