"""Launch log of a train step: every torch.ops.mog_air.* call of the SECOND
train step of a fresh model, for the batch sizes, precisions and switches at
which the weight gradients change form (mog_air/wgrads.py), one JSON line per
configuration.  Two trees that print the same digests issue the same launches
with the same arguments, on the same operands and streams.

Per call: the op, every non-tensor argument, and per tensor argument its
dtype, strides, storage offset and a storage label; the current stream.
Storages and streams are labelled by order of first appearance in the step,
so the log does not depend on addresses.  Per configuration the line holds
the launch count, the sha256 of the canonical log and the weight-gradient
launches in full.

usage: python scripts/launch_log.py OUT.jsonl [--pkg DIR] [--only SUBSTR]
  --pkg: the directory that holds the mog_air package to log (default: this
         tree's mog-asr_amd)
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "mog-asr_amd"))
    ap.add_argument("--only", default="")
    return ap.parse_args()


ARGS = _args()
sys.path[:0] = [ROOT, os.path.abspath(ARGS.pkg)]
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import mog_air  # noqa: E402  (before bench, which puts this tree's package on the path)
import bench  # noqa: E402
from mog_air.asr_model import AIRModel as AsrModel  # noqa: E402
from mog_air.ops import BF_ATOMIC, EPI_ATOMIC  # noqa: E402

DEV = torch.device("cuda:0")
WGRAD_OPS = {"wgrad_tn_x3_", "wgrad_tn_bf16_", "gemm_f32_wgrad_group_", "heads_output_wgrad_",
             "gemm_f32_x3_tn_", "gemm_x3p_tn_"}


class LaunchLog(TorchDispatchMode):
    """Forwards every op; records the mog_air ones."""

    def __init__(self):
        super().__init__()
        self.calls, self._storages, self._streams = [], {}, {}

    def _label(self, table, key):
        return table.setdefault(key, len(table))

    def _describe(self, v):
        if isinstance(v, torch.Tensor):
            return {"dtype": str(v.dtype), "strides": list(v.stride()),
                    "offset": v.storage_offset(),
                    "storage": self._label(self._storages, v.untyped_storage().data_ptr())}
        if isinstance(v, (list, tuple)):
            return [self._describe(x) for x in v]
        if isinstance(v, float):
            return repr(v)
        return v

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        ns, _, name = func._schema.name.partition("::")
        if ns == "mog_air":
            names = [a.name for a in func._schema.arguments]
            call = {"op": name, "stream": self._label(self._streams,
                                                      torch.cuda.current_stream().cuda_stream)}
            call.update({n: self._describe(v) for n, v in zip(names, args)})
            call.update({n: self._describe(v) for n, v in sorted(kwargs.items())})
            self.calls.append(call)
        return func(*args, **kwargs)


def is_wgrad(call):
    op = call["op"]
    return (op in WGRAD_OPS
            or (op == "gemm_f32_" and call["transA"] and call["epi"] == EPI_ATOMIC)
            or (op == "gemm_bf16_" and call["tn"] and call["epi"] == BF_ATOMIC))


def asr_learned(prec, scope):
    """bench.make_asr_model's configuration with the learned scale prior."""
    return AsrModel(None, None, max_steps=6, max_digits=6, rnn_units=256, canvas_size=50,
                    windows_size=28, vae_latent_dimensions=50, vae_recognition_units=(512, 256),
                    vae_generative_units=(256, 512), fix_scale_distribution=False,
                    vae_prior_mean=0.0, vae_prior_variance=1.0, vae_likelihood_std=0.0,
                    scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                    z_pres_prior_log_odds=-0.01, z_pres_temperature=0.1, stopping_threshold=0.9,
                    learning_rate=1e-4, gradient_clipping_norm=1.0, cnn=False, train=True,
                    scope=scope, annealing_schedules={}, device=DEV, seed=1235, noise_seed=1235,
                    precision=prec, constrains_num=[1, 3], constrains_margin_gamma=100.0,
                    constrains_num_element_gamma=10.0, constrains_area_minmax=[17, 23])


def configurations():
    """(name, model kind, precision, batch, switches)"""
    out = []
    for prec in ("fp32", "bf16"):
        for B in (64, 768, 1024, 8192):
            out.append(("air_%s_b%d" % (prec, B), "air", prec, B, {}))
    for sw in ({"VAE_WGRAD_X3": False}, {"REC_WGRAD_X3": False}, {"X_GRAD_X3": 0},
               {"X_GRAD_X3": 1}, {"ONE_PASS_WGRADS": True}):
        (k, v), = sw.items()
        out.append(("air_fp32_b1024_%s=%d" % (k, v), "air", "fp32", 1024, sw))
    out.append(("air_fp32_b64_WGRAD_GROUP=0", "air", "fp32", 64, {"WGRAD_GROUP": False}))
    for prec in ("fp32", "bf16"):
        for B in (64, 512, 1024, 8192):
            out.append(("asr_%s_b%d" % (prec, B), "asr", prec, B, {}))
        out.append(("asr_%s_b64_learned" % prec, "asr_learned", prec, 64, {}))
    return out


def log_one(name, kind, prec, B, switches):
    scope = "ll_" + "".join(c if c.isalnum() else "_" for c in name)
    if kind == "air":
        m = bench.make_model(prec, DEV, 1, 0, scope)
    elif kind == "asr":
        m = bench.make_asr_model(prec, DEV, scope)
    else:
        m = asr_learned(prec, scope)
    for k, v in switches.items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    x, k = bench.synthetic(B, 1234)
    X, K = torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV)
    m.train_step_async(X, K, global_batch=B)
    torch.cuda.synchronize()
    with LaunchLog() as log:
        m.train_step_async(X, K, global_batch=B)
    torch.cuda.synchronize()
    canon = "\n".join(json.dumps(c, sort_keys=True) for c in log.calls)
    del m
    torch.cuda.empty_cache()
    return {"config": name, "launches": len(log.calls),
            "sha256": hashlib.sha256(canon.encode()).hexdigest(),
            "weight_gradient_launches": [c for c in log.calls if is_wgrad(c)]}


def main():
    print("package:", os.path.dirname(mog_air.__file__), flush=True)
    with open(ARGS.out, "w") as f:
        for cfg in configurations():
            if ARGS.only not in cfg[0]:
                continue
            row = log_one(*cfg)
            f.write(json.dumps(row, sort_keys=True) + "\n")
            f.flush()
            print(row["config"], row["launches"], row["sha256"][:16],
                  len(row["weight_gradient_launches"]), flush=True)


if __name__ == "__main__":
    main()
