"""What the trainers' --resident switch buys, measured on the GPU host on
synthetic data (the offline stand-in of mog_air.datasets: 5,000 train and
1,000 test canvases of 1 or 3 objects), with the trainers' own code on both
sides (trainer.make_feed / run_test, the fp32 AIR models of
training_air_original.py):

 (a) 200 train iterations at batch 64 -- feed.next_batch() + model.step(), as
     train_loop runs them -- with the host feed (ShuffleBatcher + upload) and
     with records.DeviceFeed.  The two alternate over ROUNDS windows after a
     warm-up window each; a window is a host clock around work that ends in
     step()'s device-to-host read; the median window is reported.
 (b) one test pass over the 1,000-image test set (the whole set per launch,
     the trainers' default): run_test + evaluation on the host path, run_test
     with a DeviceEvaluator + result() on the device path, alternating, median
     of ROUNDS; split into upload (the test set's host-to-device copy, timed
     alone), metrics (evaluation() on the host; the two metric launches + the
     25-double copy on the device, timed alone) and infer (the rest).

Writes profiles/trainer_loop.json (or the path given) and prints it.  Needs a GPU (no fallback).
usage: python scripts/trainer_loop_time.py [output.json]"""
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
ITERS, ROUNDS, T = 200, 7, 6


def model(train, scope):
    from mog_air.air_model import AIRModel
    return AIRModel(max_steps=T, max_digits=T, canvas_size=50, scale_prior_variance=0.05,
                    z_pres_prior_log_odds=-0.01, learning_rate=1e-4, gradient_clipping_norm=1.0,
                    cnn=False, train=train, scope=scope, device=DEV, seed=21, noise_seed=22)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def feed_windows(args, tr_x, tr_k):
    from mog_air import trainer
    ctx = trainer.Dist()
    runs = {}
    for resident in (False, True):
        m = model(True, "looptime_train_%d" % resident)
        feed = trainer.make_feed(args, tr_x, tr_k, ctx, resident)

        def window(m=m, feed=feed):
            for _ in range(ITERS):
                x, k, nglobal = feed.next_batch()
                m.step(x, k, global_batch=nglobal)
        window()  # warm-up: every shape of the timed window
        runs[resident] = window
    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for resident in (False, True):  # alternating: both see the same machine state
            ms[resident].append(clock(runs[resident])[0])
    return {"iterations": ITERS, "batch": 64, "rounds": ROUNDS,
            "host_feed_ms": round(statistics.median(ms[False]), 3),
            "device_feed_ms": round(statistics.median(ms[True]), 3),
            "host_feed_ms_all": [round(v, 3) for v in ms[False]],
            "device_feed_ms_all": [round(v, 3) for v in ms[True]]}


def test_pass(args, tr_x, test):
    from mog_air import trainer
    from mog_air.evaluation import evaluation
    n = len(test[1])
    host_model, dev_model = model(False, "looptime_test_h"), model(False, "looptime_test_d")
    one_time, (test_dev, evaluator) = clock(
        lambda: trainer.resident_test_set(args, test, 50, dev_model))

    def host_pass():
        tl, ta, tm, sc, sh, nd = trainer.run_test(host_model, test, 50, 0)
        return evaluation(test[3], test[4], sh, sc, nd, csize=50), (sc, sh, nd)

    def dev_pass():
        trainer.run_test(dev_model, test_dev, 50, 0, evaluator)
        return evaluator.result()

    def upload():
        return (torch.as_tensor(test[0], dtype=torch.float32).to(DEV),
                torch.as_tensor(test[1]).to(DEV, torch.int32))

    def dev_metrics():
        evaluator.update(0, dev_model.rec_shifts, dev_model.rec_scales, dev_model.rec_num_digits)
        return evaluator.result()

    host_pass(), dev_pass()  # warm-up
    t = {k: [] for k in ("host", "dev", "upload", "host_metrics", "dev_metrics")}
    for _ in range(ROUNDS):
        ms, (res_h, (sc, sh, nd)) = clock(host_pass)
        t["host"].append(ms)
        ms, res_d = clock(dev_pass)
        t["dev"].append(ms)
        t["upload"].append(clock(upload)[0])
        t["host_metrics"].append(clock(lambda: evaluation(test[3], test[4], sh, sc, nd,
                                                          csize=50))[0])
        t["dev_metrics"].append(clock(dev_metrics)[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    # the two test models share seeds and call counts: the same detections
    dev = np.concatenate([res_d[0], res_d[1], res_d[2:]])
    host = np.concatenate([res_h[0], res_h[1], res_h[2:]])
    return {"images": n, "rounds": ROUNDS,
            "host": {"total_ms": round(med["host"], 3), "upload_ms": round(med["upload"], 3),
                     "metrics_ms": round(med["host_metrics"], 3),
                     "infer_ms": round(med["host"] - med["upload"] - med["host_metrics"], 3)},
            "device": {"total_ms": round(med["dev"], 3), "upload_ms": 0.0,
                       "metrics_ms": round(med["dev_metrics"], 3),
                       "infer_ms": round(med["dev"] - med["dev_metrics"], 3),
                       "one_time_upload_ms": round(one_time, 3)},
            "host_total_ms_all": [round(v, 3) for v in t["host"]],
            "device_total_ms_all": [round(v, 3) for v in t["dev"]],
            "max_abs_metric_difference": float(np.abs(dev - host).max())}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("trainer_loop_time.py needs a GPU: nothing is measured without one")
    from mog_air import trainer
    args = types.SimpleNamespace(synth_per_count=3000, data="mnist", dig_surfix="",
                                 write_synthetic=0, device=DEV, resident=1, test_batch=0)
    log = logging.getLogger("trainer_loop_time")
    tr_x, tr_k, test = trainer.load_data(args, "absent/a.tfrecords", "absent/b.tfrecords", [1, 3],
                                         log)
    assert trainer.resident_ok(args, tr_x, test, types.SimpleNamespace(max_steps=T), log)
    out = {"precision": "fp32", "max_steps": T, "device": torch.cuda.get_device_name(0),
           "train_images": len(tr_k), "feed": feed_windows(args, tr_x, tr_k),
           "test_pass": test_pass(args, tr_x, test)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                              "trainer_loop.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
