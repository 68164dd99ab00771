"""What the trainers' --graph switch buys, measured on the GPU host (DESIGN.md
§4.18), fp32, on the offline stand-in data of mog_air.datasets.

 (a) Loop cost.  200 iterations of the statements trainer.train_loop runs per
     iteration (in either style) -- feed.next_batch(), the step, the log row, and every
     20 iterations the log line's means -- for the AIR model of
     training_air_original.py (6 loop steps) and the AIR-ASR model of
     train_air_pr.py -gm 100 -gne 10, at batch 64 and 256 (both below
     SIDE_MIN_BATCH), fed by records.DeviceFeed (--resident 1) and by
     records.StreamFeed (--stream 1).  --graph 0 is model.step() (and, AIR-ASR,
     the log_variables property) with its host reads; --graph 1 is
     train_step_graphed() + LogRing.push(), drained every 20 iterations.  The
     two alternate over ROUNDS windows after a warm-up window each; a window is
     a host clock around work that ends in one device synchronise; medians and
     all rounds are reported.  --graph 0 is the loop as it was before the
     switch existed, so the alternation is the comparison against it.
 (b) ops.asr_log_row alone (T = 6, all steps executed) beside
     torch.ops.mog_air.batch_mean_ over four [B] vectors, the existing
     one-workgroup reduction: device events around each of 20 launches,
     median, at B = 64 and 8192.

Writes profiles/trainer_graph.json (or the path given) and prints it.  Needs a
GPU (no fallback).
usage: python scripts/trainer_graph_time.py [output.json]"""
import json
import logging
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mog-asr_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
ITERS, ROUNDS, T, LAUNCHES = 200, 7, 6, 20
# every model (and its captured graph) lives until the process ends: a graph
# is never destroyed while a later model captures its own
_MODELS = []


def air_model(scope):
    from mog_air.air_model import AIRModel
    return AIRModel(max_steps=T, max_digits=T, canvas_size=50, scale_prior_variance=0.05,
                    z_pres_prior_log_odds=-0.01, learning_rate=1e-4, gradient_clipping_norm=1.0,
                    cnn=False, train=True, scope=scope, device=DEV, seed=21, noise_seed=22,
                    annealing_schedules={"z_pres_prior_log_odds": {
                        "init": 10000.0, "min": 1e-9, "factor": 0.1, "iters": 3000,
                        "staircase": False, "log": True}})


def asr_model(scope):
    import bench
    return bench.make_asr_model("fp32", torch.device(DEV), scope)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def window(kind, graph, m, feed):
    """ITERS iterations of the loop body (trainer.train_loop, in ``kind``'s style)."""
    from mog_air import trainer
    every = trainer.LOG_EACH_ITERATION
    ring = trainer.LogRing(m) if graph else None
    names = m.log_names

    def run():
        rows, logged, sink = [], {}, []
        for _ in range(ITERS):
            x, k, nglobal = feed.next_batch()
            if graph:
                m.train_step_graphed(x, k, global_batch=nglobal)
                ring.push(m)
                step = m.global_step
            elif kind == "air":
                loss, acc, mse, step = m.step(x, k, global_batch=nglobal)
                rows.append([loss, acc, mse])
            else:
                _, _, _, step = m.step(x, k, global_batch=nglobal)
                for n, v in m.log_variables.items():
                    logged.setdefault(n, []).append(v)
            if step % every == 0:
                if graph and kind == "air":
                    rows.extend(ring.drain())
                elif graph:
                    for row in ring.drain():
                        for n, v in zip(names, row):
                            logged.setdefault(n, []).append(v)
                sink.append(np.mean(rows, axis=0) if kind == "air"
                            else [np.mean(logged[n]) for n in names])
                rows, logged = [], {}
        if graph:
            ring.drain()
        return sink
    return run


def loop_cost(tr_x, tr_k):
    from mog_air import records, trainer
    ctx = trainer.Dist()
    out = []
    for kind, make in (("air", air_model), ("asr", asr_model)):
        for batch in (64, 256):
            for feed_kind in ("resident", "stream"):
                runs = {}
                for graph in (0, 1):
                    m = make("graphtime_%s_%d_%s_%d" % (kind, batch, feed_kind, graph))
                    _MODELS.append(m)
                    if feed_kind == "resident":
                        feed = records.DeviceFeed(tr_x, tr_k, batch, trainer.EPOCHS,
                                                  min_after_dequeue=min(10000, len(tr_k)),
                                                  device=DEV, rank=0, world=1)
                    else:
                        a = types.SimpleNamespace(data="mnist", dig_surfix="", dig_num="13",
                                                  stream_seed=12345, device=DEV)
                        feed = trainer.stream_feed(a, ctx, batch)
                    runs[graph] = window(kind, graph, m, feed)
                    runs[graph]()  # warm-up: the capture, every shape of the timed window
                ms = {0: [], 1: []}
                for _ in range(ROUNDS):
                    for graph in (0, 1):  # alternating: both see the same machine state
                        ms[graph].append(clock(runs[graph]))
                med = {g: statistics.median(v) for g, v in ms.items()}
                case = {"model": kind, "batch": batch, "feed": feed_kind, "iterations": ITERS,
                        "rounds": ROUNDS,
                        "graph0_ms": round(med[0], 3), "graph1_ms": round(med[1], 3),
                        "graph0_ms_per_iteration": round(med[0] / ITERS, 4),
                        "graph1_ms_per_iteration": round(med[1] / ITERS, 4),
                        "graph0_spread_ms": round(max(ms[0]) - min(ms[0]), 3),
                        "graph1_ahead_by_more_than_graph0_spread":
                            bool(med[0] - med[1] > max(ms[0]) - min(ms[0])),
                        "graph0_ms_all": [round(v, 3) for v in ms[0]],
                        "graph1_ms_all": [round(v, 3) for v in ms[1]]}
                print(json.dumps(case), flush=True)
                out.append(case)
    return out


def events(fn):
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


def kernel_alone():
    from mog_air import ops
    from mog_air.asr_model import NQ, Q
    out = []
    for B in (64, 8192):
        g = torch.Generator(device=DEV).manual_seed(B)
        r = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
        arec, vkl, zmask = r(T, NQ, B), r(T, B), r(T, B)
        live = torch.ones(T + 1, device=DEV, dtype=torch.int32)
        live[T] = 0
        per = [r(B) for _ in range(8)]
        margin, means, row, mean4 = r(1), r(4), r(16), r(4)
        slots = [Q[n] for n in ("zkl", "skl", "shkl", "prn")]
        log_us, log_all = events(lambda: ops.asr_log_row(arec, vkl, zmask, live, *per, margin,
                                                         means, row, slots=slots))
        bm_us, bm_all = events(lambda: ops._ops.batch_mean_(per[0], per[1], per[2], per[3], B,
                                                            mean4))
        out.append({"B": B, "T": T, "launches": LAUNCHES,
                    "asr_log_row_us": log_us, "batch_mean_us": bm_us,
                    "ratio": round(log_us / bm_us, 2),
                    "floats_read_ratio": round((5 * T + 9) / 4, 2),
                    "asr_log_row_us_all": log_all, "batch_mean_us_all": bm_all})
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("trainer_graph_time.py needs a GPU: nothing is measured without one")
    from mog_air import trainer
    args = types.SimpleNamespace(synth_per_count=3000, data="mnist", dig_surfix="",
                                 write_synthetic=0, device=DEV)
    log = logging.getLogger("trainer_graph_time")
    tr_x, tr_k, _ = trainer.load_data(args, "absent/a.tfrecords", "absent/b.tfrecords", [1, 3],
                                      log)
    out = {"precision": "fp32", "max_steps": T, "device": torch.cuda.get_device_name(0),
           "train_images": len(tr_k), "kernel": kernel_alone(), "loop": loop_cost(tr_x, tr_k)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                              "trainer_graph.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
