"""The reference's TensorBoard summaries (training_air_original.py:223-301,
air/air_model.py:216-264, 896-993), reduced on the device and written as a
TensorBoard event file without TensorFlow.

Four fetches, all from device memory a step or an ``infer`` left behind:

- numeric: 320 scalars of the test model over the whole test set (steps,
  rec_loss, digit_acc, total_loss and the per-step scale, z_pres_prob,
  z_pres_kl, scale_kl, shift_kl, vae_kl, each as a mean per true object count
  and over all images; ops.summary_groups);
- variables: one histogram per variable (ops.summary_histograms, raw mode);
- images: the first reconstruction panels as PNGs;
- gradients: histogram, norm and mean of every variable's *applied* gradient,
  the values Adam consumed (ops.summary_histograms, applied mode).

Histogram buckets: TensorFlow's default (TF 1.12 histogram.cc), restated:
pos = 1e-12 * 1.1^k in double while < 1e20 (774 values), limits = [-DBL_MAX]
+ reversed(-pos) + [0.0] + pos + [DBL_MAX] (1551); a value goes to the first
limit greater than it.

Event file (tensorflow/core/util/event.proto, framework/summary.proto; field
numbers restated from memory, there is no TensorFlow here to check against):
  Event:          wall_time = 1 (double), step = 2 (int64), file_version = 3
                  (string), summary = 5 (Summary)
  Summary:        value = 1 (repeated Value)
  Value:          tag = 1 (string), simple_value = 2 (float), image = 4
                  (Image), histo = 5 (HistogramProto)
  HistogramProto: min, max, num, sum, sum_squares = 1..5 (double),
                  bucket_limit = 6, bucket = 7 (packed double)
  Image:          height = 1, width = 2, colorspace = 3 (int32),
                  encoded_image_string = 4 (bytes)
Records are framed as records.write_records frames them; the first record is
Event{wall_time, file_version: "brain.Event:2"}.
"""
from __future__ import annotations

import logging
import os
import socket
import struct
import sys
import time
from typing import List, Optional, Sequence

import numpy as np

from . import records
from .records import _enc_varint, _len_field

NPOS, NB = 774, 1551
DBL_MAX = sys.float_info.max
CADENCE = (50, 250, 500, 100)  # numeric, variables, images, gradients
NUM_IMAGES = 60

_LIMITS = None


def _positive_limits() -> np.ndarray:
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.asarray(pos, np.float64)


def bucket_limits() -> np.ndarray:
    """The 1551 bucket limits, float64, strictly increasing."""
    global _LIMITS
    if _LIMITS is None:
        pos = _positive_limits()
        assert len(pos) == NPOS
        _LIMITS = np.concatenate([[-DBL_MAX], -pos[::-1], [0.0], pos, [DBL_MAX]])
        _LIMITS.setflags(write=False)
    return _LIMITS


def bucket_thresholds() -> np.ndarray:
    """thr[k] = the smallest float32 above the k-th positive limit.  No limit
    is a float32 value (checked), so ``thr[k] <= |x|`` decides ``limit[k] <=
    |x|`` exactly for float32 x."""
    pos = _positive_limits()
    thr = pos.astype(np.float32)  # round to nearest
    low = thr.astype(np.float64) < pos
    thr[low] = np.nextafter(thr[low], np.float32(np.inf))
    if np.any(thr.astype(np.float64) == pos):
        raise AssertionError("a bucket limit is a float32 value")
    below = np.nextafter(thr, np.float32(-np.inf)).astype(np.float64)
    assert np.all(below < pos) and np.all(thr.astype(np.float64) > pos)
    return thr


# ------------------------------------------------------------- protobuf ----
def _double(fn: int, v: float) -> bytes:
    return _enc_varint((fn << 3) | 1) + struct.pack("<d", float(v))


def _float(fn: int, v: float) -> bytes:
    return _enc_varint((fn << 3) | 5) + struct.pack("<f", float(v))


def _int(fn: int, v: int) -> bytes:
    return _enc_varint(fn << 3) + _enc_varint(int(v))


def _packed_doubles(fn: int, vals) -> bytes:
    return _len_field(fn, np.asarray(vals, "<f8").tobytes())


def encode_histogram(stats, counts) -> bytes:
    """HistogramProto of one tensor: stats = (min, max, num, sum, sum_squares
    [, nonfinite]), counts [1551].  TensorFlow's compression of empty runs: a
    run of buckets with count <= 0 becomes one entry carrying the run's last
    limit (and a zero count), a non-empty bucket is one entry."""
    limits = bucket_limits()
    counts = np.asarray(counts)
    if counts.shape != (NB,):
        raise ValueError(f"counts must be [{NB}], got {counts.shape}")
    lim, bkt = [], []
    i = 0
    while i < NB:
        j = i
        while j < NB and counts[j] <= 0:
            j += 1
        if j > i:  # buckets i .. j - 1 are empty
            lim.append(limits[j - 1])
            bkt.append(0.0)
        if j < NB:
            lim.append(limits[j])
            bkt.append(float(counts[j]))
        i = j + 1
    return (_double(1, stats[0]) + _double(2, stats[1]) + _double(3, stats[2]) +
            _double(4, stats[3]) + _double(5, stats[4]) + _packed_doubles(6, lim) +
            _packed_doubles(7, bkt))


def scalar_value(tag: str, v: float) -> bytes:
    return _len_field(1, tag.encode("utf-8")) + _float(2, v)


def histogram_value(tag: str, stats, counts) -> bytes:
    return _len_field(1, tag.encode("utf-8")) + _len_field(5, encode_histogram(stats, counts))


def image_value(tag: str, height: int, width: int, png: bytes, colorspace: int = 3) -> bytes:
    img = _int(1, height) + _int(2, width) + _int(3, colorspace) + _len_field(4, png)
    return _len_field(1, tag.encode("utf-8")) + _len_field(4, img)


def _frame(payload: bytes) -> bytes:
    head = struct.pack("<Q", len(payload))
    return (head + struct.pack("<I", records.masked_crc(head)) + payload +
            struct.pack("<I", records.masked_crc(payload)))


class EventWriter:
    """``tf.summary.FileWriter``: <folder>/events.out.tfevents.<unix time>.<hostname>,
    one framed Event per ``add``, flushed after every event."""

    def __init__(self, folder: str):
        os.makedirs(folder, exist_ok=True)
        now = time.time()
        self.path = os.path.join(folder, "events.out.tfevents.%010d.%s" % (
            int(now), socket.gethostname()))
        self._f = open(self.path, "ab")
        self._write(_double(1, now) + _len_field(3, b"brain.Event:2"))

    def _write(self, event: bytes) -> None:
        self._f.write(_frame(event))
        self._f.flush()

    def add(self, values: Sequence[bytes], step: int) -> None:
        """One Event{wall_time, step, summary} of the given Summary.Values."""
        summary = b"".join(_len_field(1, v) for v in values)
        self._write(_double(1, time.time()) + _int(2, step) + _len_field(5, summary))

    def close(self) -> None:
        if not self._f.closed:
            self._f.close()


# ----------------------------------------------------------------- tags ----
GROUP_QUANTITIES = ("steps", "rec_loss", "digit_acc", "total_loss")
STEP_QUANTITIES = ("scale", "z_pres_prob", "z_pres_kl", "scale_kl", "shift_kl", "vae_kl")


def _by_digit_count(name: str, max_digits: int) -> List[str]:
    return [f"{name}_{g}_dig" for g in range(max_digits + 1)] + [name + "_all_dig"]


def numeric_tags(max_steps: int, max_digits: int) -> List[str]:
    """The numeric summaries' tags in the order of ops.summary_groups' rows
    and groups (air_model.py:225, 231, 251, 263)."""
    tags: List[str] = []
    for q in GROUP_QUANTITIES:
        tags += _by_digit_count(q, max_digits)
    for q in STEP_QUANTITIES:
        for i in range(max_steps):
            tags += _by_digit_count(f"{q}_{i + 1}_step", max_digits)
    return tags


def parse_cadence(text) -> tuple:
    """--summary-cadence NUM,VAR,IMG,GRAD: four positive integers."""
    try:
        vals = tuple(int(p) for p in str(text).split(","))
    except ValueError:
        vals = ()
    if len(vals) != 4 or min(vals) < 1:
        raise ValueError("--summary-cadence takes four positive integers NUM,VAR,IMG,GRAD, got %r"
                         % (text,))
    return vals


class Summaries:
    """The device buffers, the cadence and the four fetches of one run.
    ``params``: the ParamStore both models share; ``full``: False for AIR-ASR,
    whose reference has the numeric and image summaries commented out."""

    def __init__(self, folder: str, params, cadence=CADENCE, full: bool = True, log=None):
        import torch
        self.writer = EventWriter(folder)
        self.num_every, self.var_every, self.img_every, self.grad_every = cadence
        self.full = full
        self.log = log or logging.getLogger("mog_air")
        self.params = params
        dev = params.flat.device
        V = len(params.specs)
        self.names = [n for n, _ in params.specs]
        self.thr = torch.from_numpy(bucket_thresholds()).to(dev)
        self.counts = torch.empty((V, NB), dtype=torch.int32, device=dev)
        self.stats = torch.empty((V, 6), dtype=torch.float64, device=dev)
        self.denom = torch.empty((V,), dtype=torch.float32, device=dev)
        self.work = torch.empty((max(1, 6 * params.n_blocks),), dtype=torch.float64, device=dev)
        self._acc = None

    # ------------------------------------------------------ histograms ----
    def _hist(self, buf, applied_clip=None):
        from . import ops
        p = self.params
        if applied_clip is None:
            ops.summary_histograms(buf, p.t_off, p.t_len, p.t_bt, p.t_bs, p.n_blocks, self.thr,
                                   self.counts, self.stats, self.work)
        else:
            ops.summary_histograms(buf, p.t_off, p.t_len, p.t_bt, p.t_bs, p.n_blocks, self.thr,
                                   self.counts, self.stats, self.work, sumsq=p.sumsq,
                                   clip=float(applied_clip), denom=self.denom)
        stats, counts = self.stats.cpu().numpy(), self.counts.cpu().numpy()
        bad = stats[:, 5]
        if np.any(bad > 0):
            self.log.warning("summaries: %d non-finite values in %s (left out of the histograms)",
                             int(bad.sum()), [n for n, b in zip(self.names, bad) if b > 0])
        return stats, counts

    def variables(self, params, step: int) -> None:
        """One histogram per variable, tagged with its name."""
        stats, counts = self._hist(params.flat)
        self.writer.add([histogram_value(n, stats[v], counts[v])
                         for v, n in enumerate(self.names) if stats[v, 2] > 0], step)

    def gradients(self, params, clip, step: int) -> None:
        """Histogram, norm and mean of every variable's applied gradient.
        Valid after a train step and before the next one: params.grad holds
        the sanitized gradients, params.sumsq their chunk sums.  ``clip``
        None (gradient_clipping_norm=None): the gradients as they are."""
        stats, counts = self._hist(params.grad, applied_clip=clip)
        values = []
        for v, n in enumerate(self.names):
            if stats[v, 2] > 0:
                values.append(histogram_value(n + "_grad_applied", stats[v], counts[v]))
            values.append(scalar_value(n + "_grad_applied_norm", np.sqrt(stats[v, 4])))
            values.append(scalar_value(n + "_grad_applied_avg",
                                       stats[v, 3] / stats[v, 2] if stats[v, 2] > 0
                                       else float("nan")))
        self.writer.add(values, step)

    # --------------------------------------------------------- numeric ----
    def numeric(self, test_model, images, digits, batch: int, step: int) -> np.ndarray:
        """A test-model pass over the test set in chunks of ``batch`` (0: one
        chunk), the grouped sums accumulated on the device and read once.
        Returns the 320 (for 6 steps, 6 objects) means in tag order."""
        import torch

        from . import ops
        T, D = test_model.max_steps, test_model.max_digits
        n = len(digits)
        chunk = batch if batch > 0 else n
        if self._acc is None or tuple(self._acc.shape) != (4 + 6 * T, D + 2, 2):
            self._acc = torch.empty((4 + 6 * T, D + 2, 2), dtype=torch.float64,
                                    device=test_model.device)
        for s in range(0, n, chunk):
            k = digits[s:s + chunk]
            test_model.infer(images[s:s + chunk], k)
            ws = test_model._ws
            tg = torch.as_tensor(k).to(test_model.device, torch.int32).contiguous()
            ops.summary_groups(tg, ws.digits, ws.bce, ws.acc_b, ws.loss_b, ws.scale, ws.zprob,
                               ws.zkl, ws.skl, ws.shkl, ws.vkl, ws.live, D, self._acc,
                               accumulate=s > 0)
        acc = self._acc.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            means = (acc[..., 0] / acc[..., 1]).astype(np.float32).reshape(-1)
        tags = numeric_tags(T, D)
        self.writer.add([scalar_value(t, m) for t, m in zip(tags, means)], step)
        return means

    # ---------------------------------------------------------- images ----
    def images(self, test_model, images, digits, step: int, num: int = NUM_IMAGES) -> None:
        """The first ``num`` reconstruction panels, tagged reconstruction/image/<k>."""
        from .visualize import png_bytes, reconstruction_images
        test_model.infer(images, digits)
        panels = reconstruction_images(test_model, images, num=num)
        values = []
        for k, p in enumerate(panels):
            rgb = np.clip(p * 255.0 + 0.5, 0, 255).astype(np.uint8)
            values.append(image_value("reconstruction/image/%d" % k, rgb.shape[0], rgb.shape[1],
                                      png_bytes(rgb)))
        self.writer.add(values, step)

    # --------------------------------------------------------- cadence ----
    def before_step(self, step: int, test_model, images, digits, batch: int,
                    vis_n: Optional[int] = None) -> None:
        """The top of an iteration, with the pre-step ``step``
        (training_air_original.py:252-283)."""
        if step % self.num_every != 0:
            return
        var = step % self.var_every == 0
        img = var and step % self.img_every == 0
        if self.full and img:
            n = len(digits) if vis_n is None else vis_n
            self.images(test_model, images[:n], digits[:n], step)
        if var:
            self.variables(self.params, step)
        if self.full:
            self.numeric(test_model, images, digits, batch, step)

    def wants_gradients(self, pre_step: int) -> bool:
        return pre_step % self.grad_every == 0

    def scalars(self, pairs, step: int) -> None:
        """Host scalars the loop already holds (the log line's means)."""
        self.writer.add([scalar_value(t, v) for t, v in pairs], step)

    def close(self) -> None:
        self.writer.close()
