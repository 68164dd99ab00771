"""What the device canvas stream (records.StreamFeed, csrc/synth.hip) costs
and what the parent's way of feeding the same batch costs, measured on the GPU
host with the trainers' own feed classes:

 (a) StreamFeed.next_batch at 64 and 8192 images, mnist glyphs, C = 50, counts
     [1, 3];
 (b) the same with the dSprites glyphs, C = 64, counts [2, 4];
 (c) records.DeviceFeed.next_batch (ShuffleBatcher.next_indices on the host,
     index upload, ops.gather_rows) over a 20,000-image resident set at the
     same batch sizes;
 (d) 50 fp32 AIR train steps at 8192 images (feed.next_batch + model.step, as
     train_loop runs them) fed by (a) and by (c).

A window is CALLS next_batch calls (or the 50 steps) between two device
synchronisations on the host clock; the sides alternate over ROUNDS windows
after a warm-up window each and the median window is reported, per call.  The
kernel alone is timed with device events over LAUNCHES launches into
preallocated outputs and reported as bytes written per second beside the copy
bandwidth mog_copy_f4 reaches (bench.copy_bandwidth: bytes read + written).

Writes profiles/stream_time.json (or the path given) and prints it.  Needs a
GPU (no fallback).
usage: python scripts/stream_time.py [output.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mog-asr_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
CALLS, ROUNDS, LAUNCHES, STEPS, STEP_ROUNDS, RESIDENT = 20, 7, 20, 50, 3, 20000
BATCHES = (64, 8192)
CASES = {"mnist_c50_13": ("mnist", 50, [1, 3]), "dsprites_c64_24": ("dsprites", 64, [2, 4])}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(sides, rounds):
    """{name: median window ms} of callables timed in turn, after one warm-up
    window each."""
    for fn in sides.values():
        fn()
    ms = {n: [] for n in sides}
    for _ in range(rounds):
        for n, fn in sides.items():
            ms[n].append(clock(fn))
    return {n: statistics.median(v) for n, v in ms.items()}, ms


def stream_feed(case, batch):
    from mog_air import datasets, records
    kind, canvas, counts = CASES[case]
    bank, sizes, _ = datasets.glyph_bank(kind)
    return records.StreamFeed(bank, sizes, counts, canvas, batch, device=DEV)


def resident_feed(batch):
    """DeviceFeed over RESIDENT canvases of the mnist stream (what they show
    does not enter the timing), with the trainers' queue size."""
    from mog_air import records
    src = stream_feed("mnist_c50_13", RESIDENT)
    x, k, _ = src.next_batch()
    return records.DeviceFeed(x.cpu().numpy(), k.cpu().numpy(), batch, None,
                              min_after_dequeue=10000, device=DEV)


def calls(feed):
    def window():
        for _ in range(CALLS):
            feed.next_batch()
    return window


def kernel_alone(case, batch, copy_gbs):
    from mog_air import datasets, ops
    kind, canvas, counts = CASES[case]
    bank, sizes, _ = datasets.glyph_bank(kind)
    sb = ops.SynthBank(bank, sizes, counts, canvas, DEV)
    x = torch.empty((batch, canvas * canvas), device=DEV)
    k, o, s = (torch.empty(shape, dtype=torch.int32, device=DEV)
               for shape in ((batch,), (batch, 8, 5), (batch,)))
    for i in range(3):
        ops.synth_canvases(sb, 12345, i * batch, x, k, o, s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(LAUNCHES):
        ops.synth_canvases(sb, 12345, (3 + i) * batch, x, k, o, s)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / LAUNCHES
    nbytes = sum(t.numel() * t.element_size() for t in (x, k, o, s))
    return {"us_per_launch": round(us, 2), "bytes_written": nbytes,
            "written_gbs": round(nbytes / us * 1e-3, 1),
            "store_time_at_copy_rate_us": round(nbytes / copy_gbs * 1e-3, 2),
            "exhausted_images": int(s.sum())}


def train_steps():
    from mog_air.air_model import AIRModel
    sides = {}
    for name, feed in (("stream", stream_feed("mnist_c50_13", 8192)),
                       ("resident", resident_feed(8192))):
        m = AIRModel(max_steps=6, max_digits=6, canvas_size=50, scale_prior_variance=0.05,
                     z_pres_prior_log_odds=-0.01, learning_rate=1e-4, gradient_clipping_norm=1.0,
                     cnn=False, train=True, scope="streamtime_" + name, device=DEV, seed=21,
                     noise_seed=22)

        def window(m=m, feed=feed):
            for _ in range(STEPS):
                x, k, nglobal = feed.next_batch()
                m.step(x, k, global_batch=nglobal)
        sides[name] = window
    med, ms = alternate(sides, STEP_ROUNDS)
    return {"steps": STEPS, "batch": 8192, "rounds": STEP_ROUNDS,
            "stream_ms_per_step": round(med["stream"] / STEPS, 4),
            "resident_ms_per_step": round(med["resident"] / STEPS, 4),
            "stream_ms_all": [round(v / STEPS, 4) for v in ms["stream"]],
            "resident_ms_all": [round(v / STEPS, 4) for v in ms["resident"]]}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stream_time.py needs a GPU: nothing is measured without one")
    import bench
    copy_gbs = bench.copy_bandwidth(torch.device(DEV), 1.0)
    out = {"device": torch.cuda.get_device_name(0), "copy_f4_gbs": round(copy_gbs, 1),
           "calls_per_window": CALLS, "rounds": ROUNDS, "resident_images": RESIDENT,
           "next_batch": {}, "kernel": {}}
    for batch in BATCHES:
        sides = {case: calls(stream_feed(case, batch)) for case in CASES}
        sides["resident_gather"] = calls(resident_feed(batch))
        med, ms = alternate(sides, ROUNDS)
        out["next_batch"][str(batch)] = dict(
            {n + "_us": round(v / CALLS * 1e3, 2) for n, v in med.items()},
            **{n + "_us_all": [round(x / CALLS * 1e3, 2) for x in v] for n, v in ms.items()})
        for case in CASES:
            out["kernel"]["%s_%d" % (case, batch)] = kernel_alone(case, batch, copy_gbs)
    out["train_steps_fp32"] = train_steps()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                              "stream_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
