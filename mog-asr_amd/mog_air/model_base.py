"""ModelBase — what the AIR model (air_model.py) and the AIR-ASR model
(asr_model.py) share: the constructor's hyper-parameters, gates and variable
scopes, the per-batch workspace, the streams, the noise, the grouped
weight-gradient launch of a small batch, the STN write backward over all
steps and the public API (``step``, ``train_step_async``,
``compute_gradients``, ``infer``).  A model adds its loop: ``_forward``,
``_forward_loss``, ``_backward`` and ``_backward_body``.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import ops
from .graph import GraphCapture
from .params import ParamStore, WeightCache
from .results import Results
from .vae import GlimpseVAE
from .wgrads import WeightGradients

_ops = ops._ops  # torch.ops.mog_air (csrc/torch_ops.cpp)

R_NREC = 17  # step-record slots of air_cell.hip (air_model.py names them)

_SCOPES: Dict[str, ParamStore] = {}


def _f32log(v: float) -> float:
    return float(np.log(np.float32(v), dtype=np.float32))


def annealed_value(schedule: dict, global_step: int, eps=1e-9) -> float:
    """tf.train.exponential_decay (+min/max/log) in fp32 (air_model.py:164-184)."""
    f = np.float32
    p = f(global_step) / f(schedule["iters"])
    if schedule.get("staircase", False):
        p = np.floor(p)
    v = f(schedule["init"]) * np.power(f(schedule["factor"]), p, dtype=np.float32)
    if "min" in schedule:
        v = np.maximum(v, f(schedule["min"]))
    if "max" in schedule:
        v = np.minimum(v, f(schedule["max"]))
    if schedule.get("log", False):
        v = np.log(v + f(eps), dtype=np.float32)
    return float(v)


_STREAMS: Dict[torch.device, tuple] = {}


def _shared_streams(device):
    """The side stream and the third stream of the models, created once per
    process and device.  HIP places a stream on one of its GPU_MAX_HW_QUEUES
    (4) hardware queues when the stream is created; with a pair created per
    model, every other model of a process had both on ONE queue, which
    serialised the third stream behind the side stream (fp32 step 3.09 ->
    3.43 ms, bf16 2.09 -> 2.29 ms; scripts/gpu_slot_trace.sh: queues 2 / 3 for
    the first model, 4 / 4 for the second).  The first pair of a process sits
    on two queues of its own, and every model now uses it."""
    key = torch.device(device)
    if key not in _STREAMS:
        _STREAMS[key] = (torch.cuda.Stream(device=key), torch.cuda.Stream(device=key))
    return _STREAMS[key]


class _Workspace:
    """All per-batch device buffers of one train step (HBM-resident, reused),
    with the step's flags and cross-stream events.  Every field is declared
    here (or in alloc_backward) with its idle value: a buffer that only some
    schedules need is None until ``buffer`` allocates it.  Buffers in
    ZERO_PADDED carry zero pad columns written once at allocation (the bf16
    latents' 50 -> 56 columns, X's C2 -> C2p: the K padding of the GEMMs that
    read them); every other element is written by the step before it is read."""

    ZERO_PADDED = ("zb", "dmub", "dlvb", "Xb")

    def __init__(self, m: "ModelBase", B: int):
        dev = self.device = m.device
        T, H, C2, W2, Z = m.max_steps, m.rnn_units, m.C2, m.W2, m.vae_latent_dimensions
        R1, R2 = m.vae_recognition_units
        G1, G2 = m.vae_generative_units
        HS = m.scale_hidden_units
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
        self.B = B
        self.Gx = e(B, 4 * H)
        self.G = e(T, B, 4 * H)
        self.c = e(T, B, H)
        self.h = e(T, B, H)
        self.hid = e(5, T, B, HS)
        self.rec = e(T, R_NREC, B)
        self.th_f = e(T, B, 6)
        self.th_b = e(T, B, 6)
        self.scale = e(T, B)
        self.shift = e(T, B, 2)
        self.zprob, self.zkl, self.skl, self.shkl = e(T, B), e(T, B), e(T, B), e(T, B)
        self.zmask, self.zval, self.vkl = e(T, B), e(T, B), e(T, B)
        self.zc = e(T, B)
        self.bf16 = m.precision == "bf16"
        self.mu, self.lv, self.z = e(T, B, Z), e(T, B, Z), e(T, B, Z)
        self.r = e(T, B, W2)
        if self.bf16:
            eb = lambda *s: torch.empty(s, device=dev, dtype=torch.bfloat16)  # noqa: E731
            Zp = (Z + 7) // 8 * 8
            self.gb, self.a1b, self.a2b = eb(T, B, W2), eb(T, B, R1), eb(T, B, R2)
            self.zb = torch.zeros((T, B, Zp), device=dev, dtype=torch.bfloat16)
            self.d1b, self.d2b = eb(T, B, G1), eb(T, B, G2)
        else:
            self.g = e(T, B, W2)
            # (post-activations only: the softplus backward reads sigmoid(x)
            # as 1 - exp(-softplus(x)), mog_gemm_f32 epi 4)
            self.a1, self.a2 = e(T, B, R1), e(T, B, R2)
            self.d1, self.d2 = e(T, B, G1), e(T, B, G2)
        self.canvas = e(B, C2)
        # fused bf16 step: per-step canvas contributions, summed by the loss kernel
        parts = m._parts_layout(B)
        self.cparts = e(T, B, C2) if parts else None
        self.prows = torch.empty((T, B), device=dev, dtype=torch.int32) if parts else None
        self.stop, self.runloss = e(B), e(B)
        self.digits = torch.empty(B, device=dev, dtype=torch.int32)
        self.live = torch.empty(T + 1, device=dev, dtype=torch.int32)
        self.recon = e(B, C2)
        self.bce, self.mse, self.loss_b, self.acc_b = e(B), e(B), e(B), e(B)
        self.means = e(4)
        # noise
        self.eps_scale, self.eps_shift = e(T, B), e(T, B, 2)
        self.eps_z, self.eps_x, self.u = e(T, B, Z), e(T, B, W2), e(T, B)
        self.eps_x_offset = None  # set when the fused kernel generates eps_x itself
        self.noise_side = False   # this step's noise was filled on the side stream
        # the LSTM x-rows gradient's operands (buffer()): X in bf16 / in three
        # bf16 pieces, the summed dG likewise; xb_fresh: Xb holds this step's X;
        # xb_ready: the event after its conversion on the side stream
        self.Xb = self.dGsumb = self.X3 = self.dG3 = None
        self.xb_fresh = False
        self.xb_ready = None
        self.dh_parts = None  # the K slices of a small batch's dh GEMM (DH_PARTS)
        # cnn=True (AIR): the encoder's features (the LSTM input) and the
        # pooled planes its backward reads; alloc_backward: dF and the
        # per-workgroup partial sums of this batch size (a workspace is one
        # batch size's: another batch gets another workspace)
        self.feat = self.pool1 = self.pool2 = self.dF = self.cnn_part = None
        if m.cnn:
            F = m.cnn_filters
            self.feat = e(B, m.lstm_in)
            self.pool1 = e(B, ops.CNN_POOL1 ** 2 * F)
            self.pool2 = e(B, ops.CNN_POOL2 ** 2 * F)
        self._bwd = False
        self.materialized = False

    def buffer(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        """The declared buffer ``name``, allocated on first use (zero-filled
        if it is in ZERO_PADDED)."""
        buf = getattr(self, name)
        if buf is None:
            make = torch.zeros if name in self.ZERO_PADDED else torch.empty
            buf = make(shape, device=self.device, dtype=dtype)
            setattr(self, name, buf)
        return buf

    def alloc_backward(self, m: "ModelBase"):
        if self._bwd:
            return
        dev, B = m.device, self.B
        T, H, C2, W2, Z = m.max_steps, m.rnn_units, m.C2, m.W2, m.vae_latent_dimensions
        R1, R2 = m.vae_recognition_units
        G1, G2 = m.vae_generative_units
        HS = m.scale_hidden_units
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
        self.dcanvas = e(B, C2)
        if self.bf16:
            eb = lambda *s: torch.empty(s, device=dev, dtype=torch.bfloat16)  # noqa: E731
            Zp = (Z + 7) // 8 * 8
            self.dmb, self.dd2b, self.dd1b = eb(T, B, W2), eb(T, B, G2), eb(T, B, G1)
            self.dmub = torch.zeros((T, B, Zp), device=dev, dtype=torch.bfloat16)
            self.dlvb = torch.zeros((T, B, Zp), device=dev, dtype=torch.bfloat16)
            self.da2b, self.da1b = eb(T, B, R2), eb(T, B, R1)
        else:
            self.dm = e(T, B, W2)
            self.dd2, self.dd1 = e(T, B, G2), e(T, B, G1)
            self.dmu, self.dlv = e(T, B, Z), e(T, B, Z)
            self.da2, self.da1 = e(T, B, R2), e(T, B, R1)
        self.dth_f = e(B, 6)  # (AIR-ASR: one step's STN read backward)
        # all loop steps at once (AIR: only the LSTM chain is sequential)
        self.dg_all = e(T, B, W2)
        self.dz_all, self.tmp_a2_all = e(T, B, Z), e(T, B, R2)
        self.dth_f_all, self.dth_b_all, self.dot_all = e(T, B, 6), e(T, B, 6), e(T, B)
        self.dout = e(5, T, B, 2)
        # heads side by side per row ([T, B, 5, HS]): dh is one GEMM over K = 5 HS;
        # 4 HS floats of slack after it, so that head z's column view spans
        # T*B whole rows from its origin (the grouped weight-gradient kernels
        # read K x ld elements of an operand, mog_wgrad_tn_x3)
        self.dhid = e(T * B * 5 * HS + 4 * HS)[:T * B * 5 * HS].view(T, B, 5, HS)
        self.dh = e(T, B, H)
        self.dc = e(2, B, H)
        self.dG = e(T, B, 4 * H)
        self.dGsum = e(B, 4 * H)
        if m.cnn:
            self.dF = e(B, m.lstm_in)
            self.cnn_part = e(ops.cnn_partial_elems(B))
        self._bwd = True


_NO_TIMER = contextlib.nullcontext()


class _Timer:
    def __init__(self, sink, name, work):
        self.sink, self.name, self.work = sink, name, work

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        s = torch.cuda.current_stream()
        self.e0.record(s)
        # a launch on a side stream: its events also count the time its
        # first workgroups wait for CUs the main stream's kernels hold
        self.side = any(s == o for o in _STREAMS.get(s.device, ()))
        return self

    def __exit__(self, *a):
        self.e1.record(torch.cuda.current_stream())
        self.sink.setdefault(self.name, []).append((self.e0, self.e1, self.work, self.side))
        return False


class ModelBase(GlimpseVAE, WeightGradients, GraphCapture, Results):
    """See module docstring.  Keyword-only arguments beyond the reference's:
    ``device``, ``seed`` (weight init), ``noise_seed`` (device Philox noise),
    ``grad_world`` (data-parallel world size folded into the loss-mean
    gradient scale), ``precision``, ``fused_step``."""

    _SCOPE_PREFIX = "air/rnn/"  # variable scope of the loop body (air_model.py:127,812)
    _WORKSPACE = _Workspace
    num_prior = None
    marginal = None  # the ``-ap`` per-step prior bias (AIR only)
    cnn = False      # the convolutional image encoder ahead of the LSTM (AIR only)

    def __init__(self, *, input_images, target_num_digits, max_steps, max_digits, rnn_units,
                 canvas_size, windows_size, vae_latent_dimensions, vae_recognition_units,
                 vae_generative_units, scale_prior_mean, scale_prior_variance, shift_prior_mean,
                 shift_prior_variance, vae_prior_mean, vae_prior_variance, vae_likelihood_std,
                 scale_hidden_units, shift_hidden_units, z_pres_hidden_units,
                 z_pres_prior_log_odds, z_pres_temperature, stopping_threshold, learning_rate,
                 gradient_clipping_norm, num_summary_images, train, scope, annealing_schedules,
                 generation_batch_size, device, noise_seed, grad_world, precision, fused_step):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' (bit-exact parity) or 'bf16'")
        self.precision = precision
        # the fused step kernels are compiled for the reference's default VAE shape
        fused = bool(fused_step) and (
            windows_size == 28 and tuple(vae_recognition_units) == (512, 256)
            and vae_latent_dimensions == 50 and tuple(vae_generative_units) == (256, 512))
        # bf16: one fused STN-read -> VAE -> STN-write launch per loop step
        # (vae_step.hip)
        self.fused_step = fused and precision == "bf16"
        # fp32: the same fused step at the reference precision over the rows
        # of GlimpseVAE._vae_forward_all (stn_vae_step_f32_kernel;
        # fused_step=False runs the unfused sequence it is bit-identical to)
        self.fused_f32 = fused and precision == "fp32"
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise RuntimeError("AIRModel runs on a HIP device only (no CPU fallback)")
        _lib.load_torch_ops()
        self.input_images = input_images
        self.target_num_digits = target_num_digits
        self.max_steps, self.max_digits = int(max_steps), max_digits
        self.rnn_units = int(rnn_units)
        self.canvas_size, self.windows_size = int(canvas_size), int(windows_size)
        self.C2, self.W2 = self.canvas_size ** 2, self.windows_size ** 2
        # width of the LSTM's loop-invariant input: the canvas, or (AIR,
        # cnn=True) the encoder's features
        self.lstm_in = self.C2
        self.vae_latent_dimensions = int(vae_latent_dimensions)
        self.vae_recognition_units = tuple(vae_recognition_units)
        self.vae_generative_units = tuple(vae_generative_units)
        self.scale_prior_mean, self.scale_prior_variance = scale_prior_mean, scale_prior_variance
        self.shift_prior_mean, self.shift_prior_variance = shift_prior_mean, shift_prior_variance
        self.vae_prior_mean, self.vae_prior_variance = vae_prior_mean, vae_prior_variance
        self.vae_likelihood_std = vae_likelihood_std
        self.scale_hidden_units = scale_hidden_units
        self.shift_hidden_units = shift_hidden_units
        self.z_pres_hidden_units = z_pres_hidden_units
        self.z_pres_prior_log_odds = z_pres_prior_log_odds
        self.z_pres_temperature = z_pres_temperature
        self.stopping_threshold = stopping_threshold
        self.learning_rate = learning_rate
        self.gradient_clipping_norm = gradient_clipping_norm
        self.num_summary_images = num_summary_images
        self.train = bool(train)
        self.scope = scope
        self.annealing_schedules = dict(annealing_schedules or {})
        self.generation_batch_size = generation_batch_size
        self.noise_seed = int(noise_seed)
        self.grad_world = int(grad_world)
        self._noise_ctr = 0
        self.scale_prior_log_variance = _f32log(scale_prior_variance)
        self.shift_prior_log_variance = _f32log(shift_prior_variance)
        self.vae_prior_log_variance = _f32log(vae_prior_variance)
        self._ws: Optional[_Workspace] = None
        self._last_T = None
        self._outputs_ready = False

    def _bind_params(self, key: str, specs, reuse: bool, seed: int, pad=None) -> None:
        """The scope's variables: created and registered under ``key``, or
        (``reuse``) those a model of the same shapes registered there."""
        if reuse:
            if key not in _SCOPES:
                raise ValueError(f"reuse=True but scope {self.scope!r} has no variables yet")
            self.params = _SCOPES[key]
            if self.params.specs != specs:
                raise ValueError("reused scope has different variable shapes")
        else:
            self.params = _SCOPES[key] = ParamStore(specs, self.device, seed=seed, pad=pad)
        self._wcache = WeightCache(self.params)  # copies derived from the weights

    # ----------------------------------------------------------- helpers ---
    # Optional per-kernel HIP-event timing (bench.py roofline): when
    # ``kernel_events`` is a dict, every tagged launch records (start, end,
    # work, side) on the stream it is launched on; work = (bound, amount,
    # peak[, "x3"]) -- algorithmic flops ("mfma", peak "fp32" / "bf16"; "x3":
    # fp32 flops issued as six bf16 products) or bytes ("hbm") of that one
    # launch, or None (bench.kernel_work prices the tag); side: launched on
    # one of the shared side streams.
    kernel_events = None

    def _timed(self, name, work=None):
        if self.kernel_events is None:
            return _NO_TIMER
        return _Timer(self.kernel_events, name, work)

    @property
    def global_step(self) -> int:
        return self.params.global_step

    # Data parallelism (parallel.attach): the loss is the mean over the GLOBAL
    # batch, so each rank scales its loss gradient by 1/B_global and the SUM
    # all-reduce of the shards' gradients is the full-batch gradient even for
    # unequal shards.  B_global defaults to B_local * grad_world; the trainer
    # passes the true global batch of each step (global_batch=...).
    _global_batch: Optional[int] = None

    def _gscale(self, B: int) -> float:
        gb = self._global_batch if self._global_batch is not None else B * self.grad_world
        return 1.0 / float(gb)

    # set by parallel.attach: bucketed async SUM all-reduce of params.grad
    # (launch(view) as buckets become final during the backward, wait() before
    # the optimizer) and, for the data-dependent loop exit, a MAX all-reduce of
    # each step's live flag (only where the exit changes the loss: ``-ap``)
    grad_reducer = None
    live_hook = None

    def _reduce_bucket(self, lo: int, hi: int) -> None:
        if self.grad_reducer is not None:
            self.grad_reducer.launch(self.params.grad[lo:hi])

    def hyper(self, name: str) -> float:
        """Current value of a possibly-annealed hyper-parameter, evaluated at
        the pre-increment global step (as in the reference forward pass)."""
        if name in self.annealing_schedules:
            return annealed_value(self.annealing_schedules[name], self.params.global_step)
        return float(getattr(self, name))

    def _workspace(self, B: int) -> _Workspace:
        if self._ws is None or self._ws.B != B:
            self._ws = self._WORKSPACE(self, B)
        return self._ws

    def _P(self, name):
        return self.params.view(self._SCOPE_PREFIX + name)

    def _G(self, name):
        return self.params.g(self._SCOPE_PREFIX + name)

    # the step's noise on the side stream, under the x-projection: for a
    # _forward that joins it after that GEMM (AIR); False: on the current stream
    NOISE_ON_SIDE = True

    def _fill_noise(self, ws: _Workspace, noise: Optional[dict]):
        """eps_scale [T,B], eps_shift [T,B,2], eps_z, eps_x, u: injected
        (tensors or arrays), or device Philox noise."""
        ws.eps_x_offset = None  # injected noise: every consumer reads the buffers
        ws.noise_side = False
        if noise is not None:
            for k in ("eps_scale", "eps_shift", "eps_z", "eps_x", "u"):
                src = torch.as_tensor(noise[k], dtype=torch.float32)
                dst = getattr(ws, k)
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"noise[{k}] has shape {tuple(src.shape)}, "
                                     f"expected {tuple(dst.shape)}")
                dst.copy_(src)
            return
        side = None
        if self.NOISE_ON_SIDE and ws.B >= self.SIDE_MIN_BATCH:
            # on the side stream, under the x-projection (which needs none of
            # it); _forward joins it after that GEMM
            side = self._fork(self._side_stream())
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            # the step's noise buffers in one launch, each with its own Philox
            # counter range (bit-identical to one mog_rng_fill per buffer)
            outs, offs, nrm = [], [], []
            for k, normal in (("eps_scale", True), ("eps_shift", True), ("eps_z", True),
                              ("eps_x", True), ("u", False)):
                buf = getattr(ws, k)
                if k == "eps_x" and self._eps_x_in_kernel(ws.B) and not self._graph_noise:
                    # generated inside the fused step kernel / the fp32 output
                    # layer's epilogue from the same Philox counters
                    # (bit-identical to filling the buffer)
                    ws.eps_x_offset = self._noise_ctr
                else:
                    outs.append(buf)
                    offs.append(ops._i64(self._noise_ctr))
                    nrm.append(1 if normal else 0)
                self._noise_ctr += (buf.numel() + 3) // 4
            _ops.rng_fill_batch_(outs, ops._i64(self.noise_seed), offs, nrm)
        ws.noise_side = side is not None

    def _reset_loop_state(self, ws):
        """tf.while_loop's initial state (air_model.py:815-826): stopping sum,
        running loss, counts 0, live flags 1 for step 0 and 0 after (and the
        running canvas when the step does not use parts) -- one launch (a
        fill kernel: capturable, unlike a host copy)."""
        bufs = [ws.stop, ws.runloss, ws.digits, ws.live[:1], ws.live[1:]]
        vals = [0, 0, 0, 1, 0]
        if ws.cparts is None:
            bufs.append(ws.canvas)
            vals.append(0)
        _ops.fill32_batch_(bufs, vals)

    def _materialize(self):
        """Store the canvas / reconstruction of the last forward (recomputes
        the loss kernel once with its output pointers; same values)."""
        ws = self._ws
        if ws is None or ws.materialized:
            return
        X, targets = self._loss_inputs
        self._forward_loss(X, targets, ws, need_grad=False, outputs=True)

    # ---------------------------------------------------------- backward ---
    def _backward_body_grouped(self, X, ws) -> None:
        """_backward_body; small batch, one GPU: the fp32-chain weight
        gradients it meets are collected (_wgrads) and run as one grouped launch
        at the end."""
        self._wgroup = (self._wgroup_obj if (self.WGRAD_GROUP and ws.B < self.SIDE_MIN_BATCH
                                             and self.grad_reducer is None) else None)
        wg = self._wgroup
        if wg is not None:
            wg.probs = []  # (a fresh collection: nothing left from a failed step)
        try:
            self._backward_body(X, ws)
        except BaseException:
            if wg is not None:
                wg.probs = []  # a failed body's partial problems never launch
            raise
        finally:
            self._wgroup = None
        if wg is not None and wg.probs:
            flops = sum(2.0 * p[4] * p[5] * p[6] for p in wg.probs)
            with self._timed("wgrad_group", ("mfma", flops, "fp32")):
                wg.launch()

    # the grouped weight-gradient launch below SIDE_MIN_BATCH (batch 64: 11
    # launches of a few k-steps each -> one)
    WGRAD_GROUP = True
    _wgroup = None

    @property
    def _wgroup_obj(self):
        g = self.__dict__.get("_wgroup_obj_")
        if g is None:
            g = self.__dict__["_wgroup_obj_"] = ops.WgradGroup()
        return g

    def _stn_write_backward_all(self, ws) -> None:
        """Every loop step's STN write backward in one launch over T*B rows
        against the shared canvas gradient (it reads only the forward's
        records); the glimpse cotangent leaves through the VAE's output
        sigmoid straight from the kernel (dm fp32 / dmb bf16: bit-identical
        to dU followed by mog_sigmoid_backward)."""
        TB, C = self.max_steps * ws.B, self.canvas_size
        dm = ws.dmb if self.precision == "bf16" else ws.dm
        ops.stn_backward(ws.r.view(TB, -1), ws.th_b, (C, C), ws.dcanvas, gscale=ws.zc,
                         dtheta=ws.dth_b_all, dot=ws.dot_all, want_dot=True, n=TB,
                         dm=dm.view(TB, -1))

    # K-split of the small-batch dh GEMM (0: one chain per output, Cin = the
    # heads' dh)
    DH_PARTS = 4
    # the round-3 side-stream moves (noise + resets under the x-projection,
    # heads' weight gradients under the LSTM chain) from this batch: below it
    # the launches are too short to hide the cross-stream waits (batch 64:
    # eager 0.90 -> 1.00 ms, captured 0.60 -> 0.65 ms with them)
    SIDE_MIN_BATCH = 1024

    def _dh_parts(self, B: int) -> int:
        """A small batch's dh GEMM (K = 4H walked serially by a dozen
        workgroups) split over K into this many products that are added in
        part order (mog_lstm_cell_backward_parts / mog_asr_unpack_parts);
        0: one chain."""
        return self.DH_PARTS if (B < self.SIDE_MIN_BATCH and self.DH_PARTS > 1
                                 and (4 * self.rnn_units) % (4 * self.DH_PARTS) == 0) else 0

    def _stn_bwd_work(self, rows, write):
        """Algorithmic HBM bytes of one STN backward launch over `rows` image-
        steps: write -- r and dm (C2... of the glimpse), the
        canvas cotangent shared by the T steps of an image, theta / dtheta /
        dot; read -- the input canvas shared likewise, the glimpse cotangent,
        theta / dtheta."""
        W2, C2, T = self.W2, self.C2, self.max_steps
        if write:
            dm = 2 if self.precision == "bf16" else 4
            return ("hbm", rows * (W2 * 4 + W2 * dm + C2 * 4 / T + 52), None)
        return ("hbm", rows * (C2 * 4 / T + W2 * 4 + 48), None)

    # the side and third streams are created once per process and device and
    # shared by every model (see _shared_streams)
    def _stream3(self):
        return _shared_streams(self.device)[1]

    def _side_stream(self):
        return _shared_streams(self.device)[0]

    # stream-ordering test instrument (tests/test_gpu_streams.py): ticks of the
    # 100 MHz wall clock that a spin kernel holds back the head of every forked
    # segment (SPIN_FORK) or the main stream at the start of a step (SPIN_MAIN)
    SPIN_FORK = 0
    SPIN_MAIN = 0

    def _fork(self, stream):
        """Order `stream` after everything issued so far on the current
        stream; returns it."""
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        stream.wait_event(ready)
        if self.SPIN_FORK:
            with torch.cuda.stream(stream):
                ops.spin(self.SPIN_FORK)
        return stream

    # ------------------------------------------------------------- API ----
    def _prep(self, images, targets):
        X = torch.as_tensor(images, dtype=torch.float32).to(self.device).reshape(-1, self.C2)
        X = X.contiguous()
        tg = None
        if targets is not None:
            tg = torch.as_tensor(targets).to(self.device, torch.int32).contiguous()
        return X, tg

    def _begin(self, images, targets, noise, need_grad: bool, global_batch=None):
        """The inputs on the device, the workspace of their batch size and
        this step's noise."""
        X, tg = self._prep(images, targets)
        ws = self._workspace(X.shape[0])
        if need_grad:
            ws.alloc_backward(self)
            if self.SPIN_MAIN:
                ops.spin(self.SPIN_MAIN)
        self._fill_noise(ws, noise)
        if need_grad:
            self._global_batch = global_batch
        return X, tg, ws

    def train_step_async(self, images, targets=None, noise=None,
                         global_batch: Optional[int] = None) -> None:
        """One train step (forward, backward, [bucketed all-reduce], clip,
        Adam) with no host synchronisation.  ``global_batch``: images over all
        data-parallel ranks this step (default: local batch x grad_world)."""
        if not self.train:
            raise RuntimeError("train_step on a model built with train=False")
        X, tg, ws = self._begin(images, targets, noise, True, global_batch)
        self._forward(X, tg, ws, need_grad=True, outputs=False)
        self._backward(X, ws)
        if self.grad_reducer is not None:
            self.grad_reducer.wait()
        self.params.apply_adam(self.hyper("learning_rate"), self.gradient_clipping_norm)
        self.params.global_step += 1
        self._X = X

    def step(self, images, targets=None, noise=None, global_batch: Optional[int] = None):
        """``sess.run([training, loss, accuracy, mse_loss, global_step])``
        (training_air_original.py:304-310)."""
        self.train_step_async(images, targets, noise, global_batch)
        m = self._ws.means.detach().cpu().numpy()
        return float(m[0]), float(m[1]), float(m[2]), self.params.global_step

    # the trainers' log row: what ``step`` returns beside the global step
    log_names = ("loss", "accuracy", "mse")

    def _log_row_out(self, out) -> _Workspace:
        """The workspace of the last step / infer, once ``out`` is a device
        fp32 vector of len(log_names) (ValueError otherwise, nothing written)."""
        ws = self._ws
        if ws is None:
            raise RuntimeError("log_row_ before any step or infer")
        ops._chk(out, "out")
        if tuple(out.shape) != (len(self.log_names),) or out.device != ws.means.device:
            raise ValueError(f"out must be [{len(self.log_names)}] on {ws.means.device}, got "
                             f"{tuple(out.shape)} on {out.device}")
        return ws

    def log_row_(self, out: torch.Tensor) -> None:
        """The last step's (or infer's) ``log_names`` values into the device
        fp32 vector ``out`` on the current stream: one launch, no host read
        (the bits of the workspace's means; trainer.LogRing)."""
        ws = self._log_row_out(out)
        _ops.copy32_batch_([out], [ws.means[:len(self.log_names)]])

    def compute_gradients(self, images, targets=None, noise=None, canvas_cotangent=None,
                          global_batch: Optional[int] = None):
        """Forward + backward (+ the data-parallel all-reduce when attached),
        no optimizer update; returns the gradient dict.  ``canvas_cotangent``
        [B, C*C] replaces dL/dcanvas of the BCE term (used by the gradient
        parity tests)."""
        X, tg, ws = self._begin(images, targets, noise, True, global_batch)
        self._forward(X, tg, ws, need_grad=True)
        if canvas_cotangent is not None:
            ws.dcanvas.copy_(torch.as_tensor(canvas_cotangent, dtype=torch.float32))
        self._backward(X, ws)
        if self.grad_reducer is not None:
            self.grad_reducer.wait()
        return self.params.grad_dict()

    def infer(self, images, targets=None, noise=None):
        """Forward pass only (the test model's fetches)."""
        X, tg, ws = self._begin(images, targets, noise, False)
        self._forward(X, tg, ws, need_grad=False)
        self._X = X
        return self
