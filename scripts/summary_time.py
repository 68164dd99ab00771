"""What --summaries 1 costs, measured on the GPU host, fp32.

 (a) The launches alone, by device events (median of 20 after a warm-up): the
     two histogram calls of a fetch -- raw over params.flat (the variable
     summaries) and applied over params.grad (the gradient summaries) -- at
     the parameter tables of the AIR model of training_air_original.py and the
     AIR-ASR model of train_air_pr.py, and one ops.summary_groups launch at
     B = 1000, Tmax = 6.
 (b) The entry points end to end: ms per iteration of training_air_original.py
     and train_air_pr.py -gm 100 -gne 10 at batch 64 with --graph 1 --stream 1,
     --summaries 0 against --summaries 1 (the reference's cadence 50, 250, 500,
     100), alternating in fresh processes, RUNS runs each.  A run timestamps
     the feed's next_batch calls; its figure is the time from iteration 200 to
     iteration ITERS divided by the iterations between (so it includes every
     summary fetch that falls there: 20 numeric passes, 4 variable, 2 image
     and 10 gradient fetches for AIR).

Writes profiles/summary_time.json (or the path given) and prints it.  Needs a
GPU (no fallback).
usage: python scripts/summary_time.py [output.json]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mog-asr_amd"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
LAUNCHES, RUNS, ITERS, SKIP = 20, 3, 1200, 200
ENTRIES = {"air": ("training_air_original", []), "asr": ("train_air_pr", ["-gm", "100", "-gne", "10"])}


def events(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(LAUNCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(us), 2), [round(v, 2) for v in us]


def kernels():
    import torch

    import bench
    from mog_air import ops, summaries
    from mog_air.air_model import AIRModel
    out = []
    air = AIRModel(max_steps=6, max_digits=6, canvas_size=50, scale_prior_variance=0.05,
                   z_pres_prior_log_odds=-0.01, learning_rate=1e-4, gradient_clipping_norm=1.0,
                   cnn=False, train=True, scope="summtime_air", device=DEV)
    asr = bench.make_asr_model("fp32", torch.device(DEV), "summtime_asr")
    thr = torch.from_numpy(summaries.bucket_thresholds()).to(DEV)
    for name, m in (("air", air), ("asr", asr)):
        p = m.params
        V = len(p.specs)
        g = torch.Generator(device=DEV).manual_seed(V)
        p.grad.copy_(torch.randn(p.total, device=DEV, generator=g) * 1e-3)
        p.sumsq.fill_(2.0 ** -10)
        counts = torch.empty((V, summaries.NB), dtype=torch.int32, device=DEV)
        stats = torch.empty((V, 6), dtype=torch.float64, device=DEV)
        denom = torch.empty((V,), dtype=torch.float32, device=DEV)
        work = torch.empty((6 * p.n_blocks,), dtype=torch.float64, device=DEV)
        tab = (p.t_off, p.t_len, p.t_bt, p.t_bs, p.n_blocks, thr, counts, stats, work)
        raw_us, raw_all = events(lambda: ops.summary_histograms(p.flat, *tab))
        app_us, app_all = events(lambda: ops.summary_histograms(p.grad, *tab, sumsq=p.sumsq,
                                                                clip=1.0, denom=denom))
        out.append({"table": name, "tensors": V, "elements": p.n_params, "blocks": p.n_blocks,
                    "launches": LAUNCHES, "raw_us": raw_us, "applied_us": app_us,
                    "raw_GBps": round(4e-3 * p.n_params / raw_us, 1),
                    "raw_us_all": raw_all, "applied_us_all": app_all})
    B, T, D = 1000, 6, 6
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
    tg = torch.randint(0, 4, (B,), device=DEV, generator=g, dtype=torch.int32)
    st = torch.randint(0, T + 1, (B,), device=DEV, generator=g, dtype=torch.int32)
    live = torch.ones(T + 1, device=DEV, dtype=torch.int32)
    acc = torch.empty((4 + 6 * T, D + 2, 2), dtype=torch.float64, device=DEV)
    args = (tg, st, r(B), r(B), r(B)) + tuple(r(T, B) for _ in range(6)) + (live, D, acc)
    us, us_all = events(lambda: ops.summary_groups(*args))
    out.append({"groups": True, "B": B, "Tmax": T, "max_digits": D, "launches": LAUNCHES,
                "groups_us": us, "groups_us_all": us_all})
    return out


def worker(kind, summaries_on, out_path):
    """One fresh process: the entry point with the feed's next_batch calls
    timestamped (after a device synchronise at the two ends of the window)."""
    import torch

    from mog_air import records
    entry_name, flags = ENTRIES[kind]
    stamps = []
    real = records.StreamFeed.next_batch

    def next_batch(self):
        if len(stamps) in (SKIP, ITERS - 1):
            torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return real(self)
    records.StreamFeed.next_batch = next_batch
    entry = __import__(entry_name)
    folder = tempfile.mkdtemp(prefix="summary_time_")
    os.chdir(folder)
    entry.main(["-dn", "13", "--synth-per-count", "3000", "--no-images", "--iterations",
                str(ITERS), "--batch-size", "64", "--graph", "1", "--stream", "1",
                "--save-every", "0", "--summaries", str(summaries_on), "-r",
                os.path.join(folder, "res"), "-k", "t"] + flags)
    ms = (stamps[ITERS - 1] - stamps[SKIP]) * 1e3 / (ITERS - 1 - SKIP)
    with open(out_path, "w") as f:
        json.dump({"ms_per_iteration": ms}, f)


def end_to_end():
    out = []
    for kind in ENTRIES:
        ms = {0: [], 1: []}
        for _ in range(RUNS):
            for on in (0, 1):  # alternating: both see the same machine state
                with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind,
                                    str(on), tmp.name], check=True, stdout=subprocess.DEVNULL,
                                   stderr=subprocess.DEVNULL, timeout=600)
                    ms[on].append(json.load(open(tmp.name))["ms_per_iteration"])
        case = {"entry": ENTRIES[kind][0], "batch": 64, "flags": "--graph 1 --stream 1",
                "iterations": ITERS, "window": [SKIP, ITERS - 1], "runs": RUNS,
                "summaries0_ms_per_iteration": round(statistics.median(ms[0]), 4),
                "summaries1_ms_per_iteration": round(statistics.median(ms[1]), 4),
                "summaries0_all": [round(v, 4) for v in ms[0]],
                "summaries1_all": [round(v, 4) for v in ms[1]]}
        print(json.dumps(case), flush=True)
        out.append(case)
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("summary_time.py needs a GPU: nothing is measured without one")
    out = {"precision": "fp32", "device": torch.cuda.get_device_name(0), "kernels": kernels(),
           "entry_points": end_to_end()}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                              "summary_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
