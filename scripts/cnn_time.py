"""Cost of the AIR model's cnn=True image encoder: ms per fp32 train step with
cnn=False and cnn=True in the same run (B = 64 eager, B = 64 graph-captured,
B = 8192 eager; the two models alternate over ROUNDS rounds of STEPS steps
after WARMUP steps each, device events around every round, the median round
reported), and the event times of the encoder's forward and backward launches
alone at B = 8192 (median of 20 after 3), with their achieved fp32 rate
against the work they do (1.73 M / 2.96 M MAC per image) and the fp32 vector
peak.  Prints one JSON line.
usage: python scripts/cnn_time.py"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mog-asr_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

WARMUP, STEPS, ROUNDS, T = 5, 20, 5, 3
FWD_MAC, BWD_MAC = 1.73e6, 2.96e6  # per image (conv MACs; the backward with its recompute)
PEAK_FP32_VECTOR = 157.3e12        # FLOP/s, MI355X


def model(cnn, scope):
    from mog_air.air_model import AIRModel
    return AIRModel(max_steps=T, max_digits=T, canvas_size=50, scale_prior_variance=0.05,
                    z_pres_prior_log_odds=-0.01, learning_rate=1e-4, gradient_clipping_norm=1.0,
                    cnn=cnn, train=True, scope=scope, device="cuda:0", seed=21, noise_seed=22)


def window(step, x, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        step(x, k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


def step_times(B, graphed, tag):
    import bench
    x, k = bench.synthetic(B, 300)
    x, k = torch.as_tensor(x).to("cuda:0"), torch.as_tensor(k).to("cuda:0")
    steps = {}
    for cnn in (False, True):
        m = model(cnn, "cnntime_%s_%d" % (tag, cnn))
        steps[cnn] = m.train_step_graphed if graphed else m.train_step_async
        for _ in range(WARMUP):
            steps[cnn](x, k)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for cnn in (False, True):  # alternating: both see the same machine state
            ms[cnn].append(window(steps[cnn], x, k))
    return {("cnn_true" if c else "cnn_false") + "_ms": round(statistics.median(v), 4)
            for c, v in ms.items()}


def kernel_times(B):
    """The encoder's launches alone, on a model's own buffers after a step."""
    import bench
    from mog_air import ops
    x, k = bench.synthetic(B, 300)
    x, k = torch.as_tensor(x).to("cuda:0"), torch.as_tensor(k).to("cuda:0")
    m = model(True, "cnntime_kernels")
    m.train_step_async(x, k)
    ws, w, g = m._ws, m._cnn_tensors(), m._cnn_tensors("grad")
    g = [t.clone() for t in g]

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    fwd = timed(lambda: ops.cnn_enc_forward(m._X, w, ws.pool1, ws.pool2, ws.feat))
    bwd = timed(lambda: ops.cnn_enc_backward(m._X, w, ws.pool1, ws.pool2, ws.feat, ws.dF,
                                             ws.cnn_part, g))
    out = {}
    for name, ms, mac in (("forward", fwd, FWD_MAC), ("backward", bwd, BWD_MAC)):
        rate = 2.0 * mac * B / (ms * 1e-3)
        out["encoder_" + name] = {"ms": round(ms, 4), "gflop": round(2.0 * mac * B / 1e9, 2),
                                  "tflops": round(rate / 1e12, 2),
                                  "share_of_fp32_vector_peak": round(rate / PEAK_FP32_VECTOR, 4)}
    return out


def main():
    out = {"precision": "fp32", "max_steps": T, "warmup": WARMUP, "steps_per_round": STEPS,
           "rounds": ROUNDS,
           "step_b64_eager": step_times(64, False, "e64"),
           "step_b64_graphed": step_times(64, True, "g64"),
           "step_b8192_eager": step_times(8192, False, "e8192"),
           "b8192": kernel_times(8192)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
