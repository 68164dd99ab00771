"""What the train state costs, measured on the GPU host:

 (a) checkpoint.save_state / load_state wall time for the train / test pair
     of both entry points (training_air_original.py's AIR and train_air_pr.py's
     AIR-ASR, fp32, the reference shapes), median of ROUNDS, after a few steps
     so that the moments are not all zero;
 (b) the trainers' iteration loop -- scripts/trainer_loop_time.py's
     200-iteration window (feed.next_batch() + model.step(), host feed) -- for
     a tree of the parent commit and for this tree, in alternating fresh
     processes, PAIRS pairs.  The loop must not be slower than the parent by
     more than the parent's own spread over its repeats (max - min of its
     per-process medians).

The parent tree is a built checkout of the parent commit (for example
``git worktree add ../parent HEAD~1`` and a build there).

Writes profiles/checkpoint_time.json (or --out) and prints it.  Needs a GPU.
usage: python scripts/ckpt_time.py --parent PATH [--pairs 3] [--out FILE]"""
import argparse
import importlib.util
import json
import logging
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 5


def _use_tree(tree):
    for p in (tree, os.path.join(tree, "mog-asr_amd")):
        sys.path.insert(0, p)


def child(tree):
    """One fresh process: the 200-iteration windows of ``tree``'s own
    scripts/trainer_loop_time.py over ``tree``'s own package."""
    _use_tree(tree)
    spec = importlib.util.spec_from_file_location(
        "trainer_loop_time", os.path.join(tree, "scripts", "trainer_loop_time.py"))
    tlt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tlt)
    import mog_air
    from mog_air import trainer
    assert os.path.abspath(mog_air.__file__).startswith(os.path.abspath(tree) + os.sep)
    args = types.SimpleNamespace(synth_per_count=3000, data="mnist", dig_surfix="",
                                 write_synthetic=0, device=tlt.DEV, resident=1, test_batch=0)
    tr_x, tr_k, _ = trainer.load_data(args, "absent/a.tfrecords", "absent/b.tfrecords", [1, 3],
                                      logging.getLogger("ckpt_time"))
    out = tlt.feed_windows(args, tr_x, tr_k)
    print("CKPT_TIME_CHILD " + json.dumps(out), flush=True)


def loop_pairs(parent, pairs):
    runs = {"parent": [], "this": []}
    for _ in range(pairs):
        for name, tree in (("parent", parent), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("CKPT_TIME_CHILD ")][-1]
            runs[name].append(json.loads(line[len("CKPT_TIME_CHILD "):]))
    res = {"iterations": runs["this"][0]["iterations"], "batch": runs["this"][0]["batch"],
           "pairs": pairs}
    for feed in ("host_feed_ms", "device_feed_ms"):
        p = [r[feed] for r in runs["parent"]]
        t = [r[feed] for r in runs["this"]]
        res[feed] = {"parent": p, "this": t, "parent_median": statistics.median(p),
                     "this_median": statistics.median(t),
                     "parent_spread": round(max(p) - min(p), 3),
                     "slower_by": round(statistics.median(t) - statistics.median(p), 3)}
        res[feed]["within_parent_spread"] = res[feed]["slower_by"] <= res[feed]["parent_spread"]
    return res


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def state_times():
    _use_tree(ROOT)
    import numpy as np
    import torch

    import bench
    from mog_air import checkpoint
    from mog_air.air_model import AIRModel
    from mog_air.asr_model import AIRModel as AsrModel
    from mog_air.records import ShuffleBatcher
    dev = "cuda:0"
    x, k = bench.synthetic(64, 1)
    x, k = torch.as_tensor(x).to(dev), torch.as_tensor(k).to(dev)
    out = {}
    for name, cls, kw in (
            ("training_air_original", AIRModel,
             dict(scale_prior_variance=0.05, stopping_threshold=0.99, vae_likelihood_std=0.3)),
            ("train_air_pr", AsrModel,
             dict(vae_likelihood_std=0.0, z_pres_temperature=0.1, stopping_threshold=0.9,
                  constrains_num=[1, 3], constrains_margin_gamma=100.0,
                  constrains_num_element_gamma=10.0, constrains_area_minmax=[17, 23]))):
        pair = [cls(max_steps=6, max_digits=6, canvas_size=50, z_pres_prior_log_odds=-0.01,
                    learning_rate=1e-4, gradient_clipping_norm=1.0, cnn=False, train=(i == 0),
                    reuse=(i == 1), scope="ckpt_time", device=dev, **kw) for i in range(2)]
        for _ in range(3):
            pair[0].step(x, k)
        # the trainers' feed: a 10,000-example queue over 6,000 examples
        n = 6000
        feed = ShuffleBatcher(np.zeros((n, 1), np.float32), np.zeros(n, np.int32), 64, 300,
                              min_after_dequeue=min(10000, n))
        feed.next_indices()
        loop = {"step": 3, "rows": [[1.0, 0.5, 0.25]] * 3}
        with tempfile.TemporaryDirectory() as tmp:
            path = checkpoint.state_path(tmp, 3)
            save = [clock(lambda: checkpoint.save_state(path, *pair, feed=feed, loop=loop))
                    for _ in range(ROUNDS)]
            size = os.path.getsize(path)
            load = [clock(lambda: checkpoint.load_state(path, *pair, feed=feed))
                    for _ in range(ROUNDS)]
        out[name] = {"variables": pair[0].params.n_params, "file_bytes": size,
                     "save_state_ms": round(statistics.median(save), 2),
                     "load_state_ms": round(statistics.median(load), 2),
                     "save_state_ms_all": [round(v, 2) for v in save],
                     "load_state_ms_all": [round(v, 2) for v in load]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_time.json"))
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child)
    _use_tree(ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ckpt_time.py needs a GPU: nothing is measured without one")
    if a.parent is None or a.pairs < 3:
        raise SystemExit("ckpt_time.py needs --parent PATH (a built tree of the parent commit) "
                         "and at least 3 pairs")
    out = {"device": torch.cuda.get_device_name(0), "precision": "fp32", "max_steps": 6,
           "rounds": ROUNDS, "state": state_times()}
    # the loop runs in fresh processes of their own: this one's device work is done
    torch.cuda.synchronize()
    out["loop"] = loop_pairs(os.path.abspath(a.parent), a.pairs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
