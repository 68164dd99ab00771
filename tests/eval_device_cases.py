"""The random detection case shared by tests/test_eval_device_cases.py (CPU:
the case is not trivial) and tests/test_gpu_eval_device.py (GPU: the device
metrics against the host's on it), and the host-side helpers both use.

300 images (the last 16-image workgroup is ragged), T = 8 loop steps, 0..8
ground-truth boxes and 0..8 detections per image; half of the detections are
jittered copies of a ground-truth box (high IoUs around the thresholds), the
rest uniform.  The first images are the three special cases (nothing on
either side, no ground truth, no detection); one image in five has at least
six boxes and six detections.  All detection values are float32-representable,
so the fp32 and fp64 device paths see the same numbers."""
import numpy as np

from mog_air.evaluation import evaluation

N, T, CSIZE = 300, 8, 50
ABS_22_24 = 2.0 ** -46  # columns 22-24: two orders of <= 8 addends in [0, 1]


def means_bar(n):
    """N values in [0, 1] summed in two orders: the means differ by at most
    N 2^-52, plus the per-image bar of the three IoU columns."""
    return n * 2.0 ** -52 + 2.0 ** -46


def random_case(seed=20261020):
    rng = np.random.default_rng(seed)
    pos, box = [], []
    shifts = rng.uniform(-0.9, 0.9, (N, T, 2))
    scales = rng.uniform(0.1, 0.5, (N, T, 1))
    num = np.zeros(N, np.int32)
    for i in range(N):
        if i % 5 == 4:
            g, d = int(rng.integers(6, 9)), int(rng.integers(6, 9))
        else:
            g, d = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        if i < 3:
            g, d = ((0, 0), (0, 3), (3, 0))[i]
        num[i] = d
        xy = rng.integers(0, CSIZE - 20, (g, 2))
        w = rng.integers(10, 20, g)
        wh = np.stack([w, w + rng.integers(-2, 3, g)], axis=1)
        pos.append(xy.reshape(-1).astype(np.int32))
        box.append(wh.reshape(-1).astype(np.int32))
        for t in range(d):
            if g and rng.uniform() < 0.5:
                j = int(rng.integers(g))  # a jittered copy of box j (boxes may be copied twice)
                c = xy[j] + wh[j] / 2.0 + rng.uniform(-1.5, 1.5, 2)
                shifts[i, t] = c / (CSIZE / 2.0) - 1.0
                scales[i, t, 0] = (wh[j].max() / 2.0 + rng.uniform(-1.0, 1.0)) / (CSIZE / 2.0)
    shifts = shifts.astype(np.float32).astype(np.float64)
    scales = scales.astype(np.float32).astype(np.float64)
    return pos, box, shifts, scales, num


def host_per_image(pos, box, shifts, scales, num, csize=CSIZE):
    """[N, 25] of the host ``evaluation`` run on every image alone."""
    out = np.zeros((len(pos), 25))
    for i in range(len(pos)):
        p, r, gi, di, gl = evaluation([pos[i]], [box[i]], shifts[i:i + 1], scales[i:i + 1],
                                      num[i:i + 1], csize=csize)
        out[i] = np.concatenate([p, r, [gi, di, gl]])
    return out


def host_means(pos, box, shifts, scales, num, csize=CSIZE):
    p, r, gi, di, gl = evaluation(pos, box, shifts, scales, num, csize=csize)
    return np.concatenate([p, r, [gi, di, gl]])


def check_against(per_image, means, ref_rows, ref_means, label):
    """The bars of the device metrics: precision / recall columns bit-equal,
    the three IoU columns within 2^-46, the 25 means within N 2^-52 + 2^-46.
    Prints the largest deviations first; returns them."""
    n = len(ref_rows)
    d_iou = float(np.abs(per_image[:, 22:] - ref_rows[:, 22:]).max()) if n else 0.0
    d_mean = float(np.abs(means - ref_means).max())
    print(f"{label}: max |per-image IoU columns - host| = {d_iou:.3e} (bar {ABS_22_24:.3e}), "
          f"max |means - host| = {d_mean:.3e} (bar {means_bar(n):.3e})")
    np.testing.assert_array_equal(per_image[:, :22], ref_rows[:, :22], err_msg=label)
    assert d_iou <= ABS_22_24, (label, d_iou)
    assert d_mean <= means_bar(n), (label, d_mean)
    return d_iou, d_mean
