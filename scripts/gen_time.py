"""Time of one generation call at the default generation batch (G = 64,
max_steps = 3): AIR-ASR's ``generate()`` and, as the yardstick, AIR's
``generate(3)`` in the same run.  Median of 20 calls after 3 warm-up calls,
device events around each call (ASR's includes its one readback of the live
flags at the end).  Prints one JSON line.
usage: python scripts/gen_time.py [G]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mog-asr_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

WARMUP, CALLS, T = 3, 20, 3


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    from mog_air.air_model import AIRModel as Air
    from mog_air.asr_model import AIRModel as Asr
    dev = torch.device("cuda:0")
    air = Air(max_steps=T, cnn=False, train=False, scope="gentime_air", device=dev,
              generation_batch_size=G)
    out = {"G": G, "max_steps": T, "calls": CALLS, "warmup": WARMUP,
           "air_generate": timed(lambda: air.generate(T))}
    # (*_scale_prior: fix_scale_distribution=False, the scale latent from the gen_scale heads)
    for name, fix, fix_scale in (("asr_generate_learned_prior", None, True),
                                 ("asr_generate_fix_steps_3", 3, True),
                                 ("asr_generate_learned_prior_scale_prior", None, False),
                                 ("asr_generate_fix_steps_3_scale_prior", 3, False)):
        asr = Asr(max_steps=T, cnn=False, train=False, scope="gentime_" + name, device=dev,
                  stopping_threshold=0.9, z_pres_temperature=0.1, vae_likelihood_std=0.0,
                  constrains_area_minmax=(17, 23), fix_steps=fix, generation_batch_size=G,
                  fix_scale_distribution=fix_scale)
        out[name] = timed(asr.generate)
        out[name]["executed_steps"] = int(asr.generated_st_back.shape[1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
