"""What the checkpoint tests share (tests/test_gpu_checkpoint*.py, the
data-parallel worker): small train / test model pairs of every configuration,
their batches, and bit-for-bit comparisons of a model's whole train state.

B = 8 and max_steps 3 keep every case to a few launches; the z_pres prior is
annealed with ``iters`` 2, so it moves at every step and a wrong global_step
after a restore changes the very next loss."""
import numpy as np
import torch

DEV = "cuda:0"
B = 8
ANNEAL = {"z_pres_prior_log_odds": {"init": 10000.0, "min": 1e-9, "factor": 0.1, "iters": 2,
                                    "staircase": False, "log": True}}

# name -> AIRModel keywords beyond the common ones
AIR_CONFIGS = {
    "fp32": dict(precision="fp32", cnn=False),
    "bf16": dict(precision="bf16", cnn=False),
    "cnn": dict(precision="fp32", cnn=True),
    "num_prior": dict(precision="fp32", cnn=False, num_prior=[1, 3]),
}


def air_pair(config, scope, seed=21, noise_seed=22, world=1, anneal=ANNEAL):
    """(train model, test model) sharing the variables of ``scope``."""
    from mog_air.air_model import AIRModel
    kw = dict(max_steps=3, max_digits=3, canvas_size=50, scale_prior_variance=0.05,
              z_pres_prior_log_odds=-0.01, learning_rate=1e-3, gradient_clipping_norm=1.0,
              scope=scope, device=DEV, annealing_schedules=anneal, seed=seed,
              noise_seed=noise_seed, generation_batch_size=4, **AIR_CONFIGS[config])
    return (AIRModel(train=True, grad_world=world, **kw),
            AIRModel(train=False, reuse=True, **kw))


def asr_pair(scope, seed=21, noise_seed=22, world=1, precision="fp32"):
    from mog_air.asr_model import AIRModel
    kw = dict(max_steps=3, max_digits=3, canvas_size=50, vae_likelihood_std=0.0,
              z_pres_prior_log_odds=-0.01, z_pres_temperature=0.1, stopping_threshold=0.9,
              learning_rate=1e-3, gradient_clipping_norm=1.0, cnn=False, scope=scope,
              constrains_num=[1, 3], constrains_margin_gamma=100.0,
              constrains_num_element_gamma=10.0, constrains_area_minmax=[17, 23],
              annealing_schedules={}, device=DEV, seed=seed, noise_seed=noise_seed,
              precision=precision, generation_batch_size=4)
    return (AIRModel(train=True, grad_world=world, **kw),
            AIRModel(train=False, reuse=True, **kw))


_BATCHES = {}


def batches(n, batch=B):
    """The first ``n`` device batches (x, k) of the fixed stream, made once."""
    import bench
    have = _BATCHES.setdefault(batch, [])
    for i in range(len(have), n):
        x, k = bench.synthetic(batch, 700 + i)
        have.append((torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV)))
    return have[:n]


def fixed_batch(batch=B):
    """The batch the test models infer on (not one of the train stream's)."""
    if ("fixed", batch) not in _BATCHES:
        import bench
        x, k = bench.synthetic(batch, 699)
        _BATCHES[("fixed", batch)] = (torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV))
    return _BATCHES[("fixed", batch)]


def snapshot(train_model, test_model=None):
    """Host copies of everything a restore must reproduce (bit patterns)."""
    p = train_model.params
    torch.cuda.synchronize()
    out = {n: getattr(p, n).detach().view(torch.int32).cpu().numpy().copy()
           for n in ("flat", "m", "v")}
    out["scalars"] = (np.float32(p.beta1_power).tobytes(), np.float32(p.beta2_power).tobytes(),
                      int(p.adam_t), int(p.global_step), int(train_model._noise_ctr),
                      None if test_model is None else int(test_model._noise_ctr))
    return out


def assert_same(a, b, what):
    assert a["scalars"] == b["scalars"], (what, a["scalars"], b["scalars"])
    for n in ("flat", "m", "v"):
        np.testing.assert_array_equal(a[n], b[n], err_msg=f"{what}: {n}")


def bits(t):
    """A device tensor's bit pattern on the host."""
    t = t.detach().contiguous()
    return t.view(torch.int32).cpu().numpy().copy() if t.dtype == torch.float32 \
        else t.cpu().numpy().copy()


def infer_outputs(test_model, generate_args=(2,)):
    """The test model's fetches on the fixed batch, then a generation: all
    noise comes from its own Philox offset."""
    x, k = fixed_batch()
    test_model.infer(x, k)
    # means: loss, accuracy, mse (the fourth slot is not written by a forward)
    out = {"means": bits(test_model._ws.means[:3]), "digits": bits(test_model.rec_num_digits),
           "loss_b": bits(test_model.per_image_loss), "recon": bits(test_model.reconstruction)}
    out["generated"] = bits(test_model.generate(*generate_args))
    out["ctr"] = np.array([test_model._noise_ctr])
    return out


def assert_outputs_equal(a, b, what):
    assert sorted(a) == sorted(b)
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=f"{what}: {n}")
