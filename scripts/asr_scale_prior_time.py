"""Cost of the learned scale prior (fix_scale_distribution=False) on the
AIR-ASR train step: the bench's configs[2] step at B = 8192 in fp32 and bf16,
and the captured batch-64 step, the fixed and the learned prior alternating,
each twice, in one process.  Device events around STEPS steps after WARMUP.
Prints one JSON document (and writes it to argv[1] when given).
usage: python scripts/asr_scale_prior_time.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mog-asr_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from mog_air.asr_model import AIRModel  # noqa: E402

STEPS, WARMUP = 10, 3
dev = torch.device("cuda:0")


def model(prec, learned, scope):
    # bench.make_asr_model's configuration (configs[2]) with the flag
    return AIRModel(None, None, max_steps=6, max_digits=6, rnn_units=256, canvas_size=50,
                    windows_size=28, vae_latent_dimensions=50, vae_recognition_units=(512, 256),
                    vae_generative_units=(256, 512), fix_scale_distribution=not learned,
                    vae_likelihood_std=0.0, z_pres_prior_log_odds=-0.01, z_pres_temperature=0.1,
                    stopping_threshold=0.9, learning_rate=1e-4, gradient_clipping_norm=1.0,
                    cnn=False, train=True, scope=scope, annealing_schedules={}, device=dev,
                    seed=1235, noise_seed=1235, precision=prec, constrains_num=[1, 3],
                    constrains_margin_gamma=100.0, constrains_num_element_gamma=10.0,
                    constrains_area_minmax=[17, 23])


def timed(prec, B, learned, graph):
    m = model(prec, learned, "sptime")
    x, k = bench.synthetic(B, 1234)
    X, K = torch.from_numpy(x).to(dev), torch.from_numpy(k).to(dev)
    step = m.train_step_graphed if graph else m.train_step_async
    for _ in range(WARMUP + (2 if graph else 0)):  # (the first graphed step runs eagerly)
        step(X, K)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        step(X, K)
    b.record()
    b.synchronize()
    loss = float(m._ws.means[0])
    del m
    return a.elapsed_time(b) / STEPS, loss


def main():
    out = {"steps": STEPS, "warmup": WARMUP, "rows": []}
    for name, prec, B, graph in (("configs2_fp32_8192", "fp32", 8192, False),
                                 ("configs2_bf16_8192", "bf16", 8192, False),
                                 ("captured_fp32_64", "fp32", 64, True)):
        ms = {False: [], True: []}
        for rep in range(2):
            for learned in (False, True):
                t, loss = timed(prec, B, learned, graph)
                assert loss == loss, "loss is NaN"
                ms[learned].append(round(t, 4))
                print(name, "learned" if learned else "fixed", rep, f"{t:.4f} ms", flush=True)
        fx, ln = ms[False], ms[True]
        out["rows"].append({"step": name, "fixed_ms": fx, "learned_ms": ln,
                            "learned_minus_fixed_ms": round(sum(ln) / 2 - sum(fx) / 2, 4),
                            "repeat_spread_ms": round(max(abs(fx[0] - fx[1]),
                                                          abs(ln[0] - ln[1])), 4)})
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
