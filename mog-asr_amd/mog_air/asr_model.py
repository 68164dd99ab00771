"""AIRModel of AIR-ASR — drop-in host object for the reference's
air/air_number_bbox_location.py:13-1361 (the model train_air_pr.py builds),
running on MI355X HIP kernels: the inference and generative LSTMCells (fp32
MFMA GEMMs with the loop-invariant x-projection hoisted), the heads and the
structural regularisers (asr_cell.hip), and the glimpse path shared with the
AIR model (STN read, glimpse VAE — fused bf16 step kernel or fp32 GEMMs —,
STN write, reconstruction loss).

Reference surface kept (air_number_bbox_location.py:15-56, train_air_pr.py:
160-213): the constructor keyword arguments (cnn=True is rejected: the entry
point does not use it), the train / test pair sharing one scope via
``reuse``, the loss of :1078-1079 with every regulariser, and the result
attributes (``loss, accuracy, mse_loss, rec_num_digits, rec_scales,
rec_shifts, rec_st_back, rec_windows, rec_latents, z_pres_probs,
reconstruction, log_variables``).

Loop: max_steps iterations on the device, the data-dependent predicate
(:386-390) folded into a live flag per step; losses, counts and gradients
equal the early exit.  The KL records are summed per type over the executed
steps at the end, as the reference's TensorArrays are (:917-923).

Scale prior: the constant N(-1, 0.05) with ``fix_scale_distribution=True``
(:70-72); with False the ``gen_scale`` heads on concat([hg_t, shift_latent])
(:482-509) give a Gaussian per image and step, and the scale KL (:729-746) is
taken against it (the learned variants of the step kernels: two more hidden
layers finished in the kernel, record slots gcm / gclv, douts columns 12 /
13).  The prior enters only that KL: every other forward output has the bits
of the fixed prior.

Generation (:1124-1361): ``generate()`` runs the generative LSTMCell as the
prior over positions and counts (asr_gen.hip), the same fixed-T schedule;
with the learned scale prior the scale latent is drawn from the gen_scale
heads on the generated shift latent (:1170-1201) and feeds the next step's
LSTM input.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .model_base import ModelBase, _Workspace
from .ops import EPI_RELU, EPI_SIGMOID_NOISE, EPI_SOFTPLUS, EPI_STORE, gemm
from .vae import _step_rows
from .wgrads import WgradProblem

_ops = ops._ops  # torch.ops.mog_air (csrc/torch_ops.cpp)

# asr_cell.hip record slots
Q = {n: i for i, n in enumerate(
    ("sm0 sm1 slv0 slv1 sl0 sl1 cm clv cl s tx ty gsm0 gsm1 gslv0 gslv1 plo lo y z act_old act "
     "live zkl skl shkl prn zprob gcm gclv").split())}
NQ = 30   # (gcm / gclv: written with the learned scale prior only)
D_N = 12  # douts columns; D_NL with the learned scale prior (+ d gcm, d gclv)
D_NL = 14
LU = 312  # packed LSTM-input row: z (50) | latents (3) | h (256) | pad (3)

ROOT = "air/air_model/"


def asr_param_specs(C2, H, W2, R, G, Z, HS, HZ, learned_scale_prior=False):
    """(TF variable name, shape): inference / generative LSTMCell kernels on
    the concatenated inputs, tf.layers.dense heads numbered in creation order
    within their scopes (:414-474, :590-609), the glimpse VAE (vae.py); with
    ``learned_scale_prior`` the gen_scale heads (:482-509) at the end, so every
    other variable keeps its offset and seeded draw in both modes."""
    p = ROOT
    specs = [(p + "infer_rnn_running/kernel", (C2 + Z + 3 + H, 4 * H)),
             (p + "infer_rnn_running/bias", (4 * H,)),
             (p + "gen_rnn_running/kernel", (Z + 3 + H, 4 * H)),
             (p + "gen_rnn_running/bias", (4 * H,))]

    def four(scope, kin, kout, extra):
        return [(p + scope + "/dense/kernel", (kin, HS)), (p + scope + "/dense/bias", (HS,)),
                (p + scope + "/dense_1/kernel", (HS + extra, kout)),
                (p + scope + "/dense_1/bias", (kout,)),
                (p + scope + "/dense_2/kernel", (kin, HS)), (p + scope + "/dense_2/bias", (HS,)),
                (p + scope + "/dense_3/kernel", (HS + extra, kout)),
                (p + scope + "/dense_3/bias", (kout,))]

    specs += four("inf_shift", H, 2, 0) + four("inf_scale", H + 2, 1, 2) + four("gen_shift", H, 2, 0)
    for scope in ("z_pres/prior", "z_pres/log_odds"):
        specs += [(p + scope + "/dense/kernel", (H, HZ)), (p + scope + "/dense/bias", (HZ,)),
                  (p + scope + "/dense_1/kernel", (HZ, 1)), (p + scope + "/dense_1/bias", (1,))]
    v = p + "vae/"
    R1, R2 = R
    G1, G2 = G
    specs += [(v + "recognition_1/weights", (W2, R1)), (v + "recognition_1/biases", (R1,)),
              (v + "recognition_2/weights", (R1, R2)), (v + "recognition_2/biases", (R2,)),
              (v + "rec_mean/weights", (R2, Z)), (v + "rec_mean/biases", (Z,)),
              (v + "rec_log_variance/weights", (R2, Z)), (v + "rec_log_variance/biases", (Z,)),
              (v + "generative_1/weights", (Z, G1)), (v + "generative_1/biases", (G1,)),
              (v + "generative_2/weights", (G1, G2)), (v + "generative_2/biases", (G2,)),
              (v + "gen_mean/weights", (G2, W2)), (v + "gen_mean/biases", (W2,))]
    if learned_scale_prior:
        specs += four("gen_scale", H + 2, 1, 2)
    return specs


class _AsrWorkspace(_Workspace):
    def __init__(self, m: "AIRModel", B: int):
        super().__init__(m, B)
        dev = m.device
        T, H = m.max_steps, m.rnn_units
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
        self.U, self.Ug = e(T, B, LU), e(T, B, LU)
        self.Gg, self.cg, self.hg = e(T, B, 4 * H), e(T, B, H), e(T, B, H)
        self.hid8 = e(m._nhid, T, B, 64)
        self.arec = e(T, NQ, B)
        self.ss = e(T, B, 3)
        self.zc = e(T, B)
        self.klsum, self.pr, self.element = e(B), e(B), e(B)
        self.area, self.outl, self.size, self.over = e(B), e(B), e(B), e(B)
        self.zsum = e(T)
        self.margin = e(1)
        # hg_{-1}: the zero state the learned prior reads at step 0
        self.hg_zero = torch.zeros((B, H), device=dev, dtype=torch.float32)
        self.x3_ready = None  # the event after X's split on the side stream (_x3_asr)
        # this step's VAE / recurrent-rows weight gradients ran per loop step
        self.vae_wgrads_done = self.u_wgrads_done = False
        self.dUp = self.dUgp = None  # the K slices of a small batch's dU / dUg GEMM (DH_PARTS)

    def alloc_backward(self, m):
        if self._bwd:
            return
        super().alloc_backward(m)
        dev, B = m.device, self.B
        T, H = m.max_steps, m.rnn_units
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
        self.dreg = e(T, 4, B)
        self.douts = e(T, B, m._dn)
        self.dpre = e(m._nhid, T, B, 64)
        self.dhg = e(T, B, H)
        self.dcg = e(2, B, H)
        self.dGg = e(T, B, 4 * H)
        self.dGgsum = e(B, 4 * H)
        self.dU, self.dUg = e(B, LU), e(B, LU)
        self.dss_carry = e(B, 3)


class AIRModel(ModelBase):
    """See module docstring.  Extra keyword-only arguments as the AIR model
    (device, seed, noise_seed, grad_world, precision, fused_step)."""

    NOISE_ON_SIDE = False  # _forward below uses the noise from its first launch

    _SCOPE_PREFIX = ROOT
    _WORKSPACE = _AsrWorkspace

    def __init__(self, input_images=None, target_num_digits=None, max_steps=3, max_digits=2,
                 rnn_units=256, canvas_size=50, windows_size=28, vae_latent_dimensions=50,
                 vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                 fix_scale_distribution=True, vae_prior_mean=0.0, vae_prior_variance=1.0,
                 vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64,
                 z_pres_hidden_units=64, z_pres_prior_log_odds=-2.0, z_pres_temperature=1.0,
                 stopping_threshold=0.99, learning_rate=1e-3, gradient_clipping_norm=100.0,
                 cnn=True, cnn_filters=8, num_summary_images=60, train=False, reuse=False,
                 scope="air", annealing_schedules=None, generation_batch_size=64,
                 reuse_shift_scale_network=True, constrains_x_y=None, constrains_num=None,
                 constrains_num_gamma=0.0, constrains_bbox_gamma=0.0, constrains_margin_gamma=0.0,
                 constrains_num_element_gamma=0.0, constrains_sharesize_gamma=0.0,
                 constrains_area_gamma=0.0, constrains_area_minmax=(0.0, 0.0), fix_steps=None, *,
                 device=None, seed: int = 1235, noise_seed: int = 1235, grad_world: int = 1,
                 precision: str = "fp32", fused_step: bool = True):
        if cnn:
            raise NotImplementedError("cnn=True is outside the hot-path scope (train_air_pr.py "
                                      "uses cnn=False)")
        if not (scale_hidden_units == shift_hidden_units == z_pres_hidden_units == 64):
            raise NotImplementedError("the ASR heads are compiled for 64 hidden units")
        if rnn_units + vae_latent_dimensions + 3 > LU:
            raise NotImplementedError("rnn_units + latent + 3 must fit the packed input row")
        if max_steps > 8:
            raise NotImplementedError("at most 8 loop steps (regulariser kernels)")
        cons = list(constrains_num) if constrains_num is not None else [max_steps]
        if not 1 <= len(cons) <= 8:
            raise ValueError("1..8 allowed object counts")
        # the scale prior is fixed (:70-72) or the gen_scale heads'; the shift
        # prior is generation's only
        # (before the base constructor: the workspace reads them)
        self.fix_scale_distribution = bool(fix_scale_distribution)
        self._nhid = 8 if self.fix_scale_distribution else 10
        self._dn = D_N if self.fix_scale_distribution else D_NL
        super().__init__(
            input_images=input_images, target_num_digits=target_num_digits, max_steps=max_steps,
            max_digits=max_digits, rnn_units=rnn_units, canvas_size=canvas_size,
            windows_size=windows_size, vae_latent_dimensions=vae_latent_dimensions,
            vae_recognition_units=vae_recognition_units, vae_generative_units=vae_generative_units,
            scale_prior_mean=-1.0, scale_prior_variance=0.05, shift_prior_mean=0.0,
            shift_prior_variance=1.0, vae_prior_mean=vae_prior_mean,
            vae_prior_variance=vae_prior_variance, vae_likelihood_std=vae_likelihood_std,
            scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
            z_pres_prior_log_odds=z_pres_prior_log_odds, z_pres_temperature=z_pres_temperature,
            stopping_threshold=stopping_threshold, learning_rate=learning_rate,
            gradient_clipping_norm=gradient_clipping_norm, num_summary_images=num_summary_images,
            train=train, scope=scope, annealing_schedules=annealing_schedules,
            generation_batch_size=generation_batch_size, device=device, noise_seed=noise_seed,
            grad_world=grad_world, precision=precision, fused_step=fused_step)
        self.fix_steps = fix_steps
        self._fix = -1 if fix_steps is None else int(fix_steps)  # (the kernels' form)
        self.constrains_num = cons
        self._cons = [int(c) for c in cons]
        self.constrains_num_gamma = constrains_num_gamma
        self.constrains_margin_gamma = constrains_margin_gamma
        self.constrains_num_element_gamma = constrains_num_element_gamma
        self.constrains_bbox_gamma = constrains_bbox_gamma
        self.constrains_sharesize_gamma = constrains_sharesize_gamma
        self.constrains_area_gamma = constrains_area_gamma
        self.constrains_area_minmax = tuple(float(v) for v in constrains_area_minmax)
        # the LSTM GEMMs run over LU = 312 packed rows (16-byte operand
        # rows): 3 zero rows behind each LSTM kernel are the rows past its
        # Z + 3 + H, so no launch reads or accumulates into a neighbour
        kpad = (LU - (self.vae_latent_dimensions + 3 + self.rnn_units)) * 4 * self.rnn_units
        self._bind_params("asr:" + scope, asr_param_specs(
            self.C2, self.rnn_units, self.W2, self.vae_recognition_units,
            self.vae_generative_units, self.vae_latent_dimensions, 64, 64,
            not self.fix_scale_distribution), reuse, seed,
            pad={ROOT + "infer_rnn_running/kernel": kpad, ROOT + "gen_rnn_running/kernel": kpad})

    # zsum_hook / live_hook: data-parallel collectives (parallel.attach)
    zsum_hook = None

    def _Kpad(self, name, buf="flat"):
        """An LSTM kernel with its zero pad rows: [rows + pad, 4H] (the GEMMs
        over LU packed rows read / accumulate rows up to C2 + LU)."""
        key = ("kpad", buf, name)
        hit = self.params._views.get(key)
        t = getattr(self.params, buf)
        if hit is not None and hit[0] is t:
            return hit[1]
        o = self.params.offsets[ROOT + name]
        rows, cols = self.params.shapes[ROOT + name]
        pad_rows = LU - (self.vae_latent_dimensions + 3 + self.rnn_units)
        v = t[o:o + (rows + pad_rows) * cols].view(rows + pad_rows, cols)
        self.params._views[key] = (t, v)
        return v

    _OUT_W = ("inf_shift/dense_1", "inf_shift/dense_3", "inf_scale/dense", "inf_scale/dense_1",
              "inf_scale/dense_2", "inf_scale/dense_3", "gen_shift/dense_1", "gen_shift/dense_3",
              "z_pres/prior/dense_1", "z_pres/log_odds/dense_1")

    def _w20(self):
        ts = []
        for n in self._OUT_W:
            ts += [self._P(n + "/kernel"), self._P(n + "/bias")]
        return ts

    _GEN_SCALE_W = ("gen_scale/dense", "gen_scale/dense_1", "gen_scale/dense_2",
                    "gen_scale/dense_3")

    def _gw8(self):
        """The learned scale prior's eight tensors in the kernels' order."""
        return [self._P(n + s) for n in self._GEN_SCALE_W for s in ("/kernel", "/bias")]

    def _gammas(self):
        return [float(v) for v in (
            self.hyper("constrains_num_gamma"), self.hyper("constrains_margin_gamma"),
            self.hyper("constrains_num_element_gamma"), self.hyper("constrains_bbox_gamma"),
            self.hyper("constrains_sharesize_gamma"), self.hyper("constrains_area_gamma"),
            self.constrains_area_minmax[0], self.constrains_area_minmax[1])]

    # ---------------------------------------------------------- forward ---
    def _f32_parts(self, B: int) -> bool:
        """fp32 with B >= FUSED_F32_MIN_ROWS: each step's VAE is the fused fp32
        step kernel over that step's rows (GlimpseVAE._vae_forward_all), writing
        the step's canvas part (summed in step order by the loss kernel: the
        running canvas bit for bit).  Smaller batches keep the per-step
        launches (the fused kernel would leave most CUs idle, and the extra
        host work of the parts path shows at the reference's batch of 64)."""
        return self.precision == "fp32" and self.fused_f32 and B >= self.FUSED_F32_MIN_ROWS

    def _parts_layout(self, B: int) -> bool:
        return self.fused_step or self._f32_parts(B)

    def _eps_x_in_kernel(self, B: int) -> bool:
        return self.fused_step or self._f32_parts(B)

    def _batched_vae(self, B: int) -> bool:
        return False  # per step: the ASR loop feeds z of step t into step t+1's input

    def _x3_asr(self, B: int) -> bool:
        """fp32: the inference LSTM's x-rows weight gradient X^T dGsum on the
        three-piece bf16-core form (X_GRAD_X3 = 2, the default, as for AIR)
        from the batch where the side stream pays (SIDE_MIN_BATCH)."""
        return self.precision == "fp32" and self.X_GRAD_X3 == 2 and B >= self.SIDE_MIN_BATCH

    def _forward(self, X, targets, ws, need_grad, outputs=True):
        B, T, H, Z = ws.B, self.max_steps, self.rnn_units, self.vae_latent_dimensions
        C, W, C2 = self.canvas_size, self.windows_size, self.C2
        Ki = self._Kpad("infer_rnn_running/kernel")
        Kg = self._Kpad("gen_rnn_running/kernel")
        bi, bg = self._P("infer_rnn_running/bias"), self._P("gen_rnn_running/bias")
        self._reset_loop_state(ws)
        thr = self.hyper("stopping_threshold")
        temp = self.hyper("z_pres_temperature")
        lik_std = float(self.hyper("vae_likelihood_std"))
        fix = self._fix
        w20 = self._w20()
        x3 = need_grad and self._x3_asr(B)
        if x3:
            # the x-rows gradient's A operand split into three bf16 pieces on
            # the side stream, under the x-projection (the AIR model's _forward does
            # the same); joined in _weight_grads
            side = self._fork(self._side_stream())
            with torch.cuda.stream(side):
                self._x_split3(X, ws)
                ws.x3_ready = torch.cuda.Event()
                ws.x3_ready.record(side)
        elif need_grad and self.precision == "bf16" and B >= self.SIDE_MIN_BATCH:
            # bf16: X converted once for the x-rows gradient, likewise
            with torch.cuda.stream(self._fork(self._side_stream())):
                self._x_bf16(X, ws)
                ws.xb_ready = torch.cuda.Event()
                ws.xb_ready.record(torch.cuda.current_stream())
        # loop-invariant x-projection of the inference LSTM (chain over x first)
        with self._timed("lstm_x_projection"):
            gemm([X], [Ki[:C2]], [ws.Gx], B, 4 * H, C2, C2, 4 * H, 4 * H)
        relu_w = [self._P(n + "/kernel") for n in ("inf_shift/dense", "inf_shift/dense_2",
                                                   "z_pres/log_odds/dense")]
        relu_b = [self._P(n + "/bias") for n in ("inf_shift/dense", "inf_shift/dense_2",
                                                 "z_pres/log_odds/dense")]
        gen_w = [self._P(n + "/kernel") for n in ("gen_shift/dense", "gen_shift/dense_2")]
        gen_b = [self._P(n + "/bias") for n in ("gen_shift/dense", "gen_shift/dense_2")]
        sc_w = [self._P("inf_scale/dense/kernel")[:H], self._P("inf_scale/dense_2/kernel")[:H]]
        learned = not self.fix_scale_distribution
        nh = self._nhid
        if learned:
            # the gen_scale hidden layers' chains over hg_t join the same launch
            sc_w += [self._P("gen_scale/dense/kernel")[:H], self._P("gen_scale/dense_2/kernel")[:H]]
            gw8 = self._gw8()
        defer = self.precision == "fp32" and self.DEFER_DECODER
        for t in range(T):
            prev = t > 0
            # both cells' input rows in one launch
            _ops.asr_pack_(B, Z, H, LU, ws.z[t - 1] if prev else None,
                           ws.ss[t - 1] if prev else None, ws.h[t - 1] if prev else None, ws.U[t],
                           ws.hg[t - 1] if prev else None, ws.Ug[t])
            # K = LU: the packed rows end in zeros, so the chain's last terms are
            # 0 * w (exactly +-0: the sum is unchanged bit for bit) and the
            # operands are 16-byte rows (LDS-DMA GEMM); the 3 weight rows past
            # the U-part are the kernels' own zero pad rows (ParamStore pad)
            # (both LSTMCells' gate GEMMs in one batched launch; the inference
            # cell continues the hoisted x-projection's chain through Cin)
            gemm([ws.U[t], ws.Ug[t]], [Ki[C2:], Kg], [ws.G[t], ws.Gg[t]], B, 4 * H, LU, LU,
                 4 * H, 4 * H, bias=[bi, bg], Cin=[ws.Gx, None])
            # (both cells' gates in one launch)
            _ops.lstm_cell_forward2_(ws.G[t], ws.c[t - 1] if prev else None, ws.c[t], ws.h[t],
                                     ws.Gg[t], ws.cg[t - 1] if prev else None, ws.cg[t],
                                     ws.hg[t], B, H)
            hid = [ws.hid8[k, t] for k in range(nh)]
            # (the inference and generative ReLU heads in one batched launch, with
            # the learned prior from the previous generative output (:596-602):
            # hg_{t-1}, the rows asr_pack_ copied into Ug[t])
            ra, rw = [ws.h[t]] * 3 + [ws.hg[t]] * 2, list(relu_w) + list(gen_w)
            rb = list(relu_b) + list(gen_b)
            if fix < 0:
                ra.append(ws.hg[t - 1] if prev else ws.hg_zero)
                rw.append(self._P("z_pres/prior/dense/kernel"))
                rb.append(self._P("z_pres/prior/dense/bias"))
            gemm(ra, rw, hid[0:len(ra)], B, 64, H, H, 64, 64, epi=EPI_RELU, bias=rb)
            gemm([ws.h[t]] * 2 + [ws.hg[t]] * (nh - 8), sc_w, hid[6:nh], B, 64, H, H, 64, 64,
                 epi=EPI_STORE)
            hid_l = [x if (k != 5 or fix < 0) else None for k, x in enumerate(hid)]
            outs = (ws.eps_shift[t], ws.eps_scale[t], ws.u[t], ws.stop, ws.digits, ws.live,
                    ws.arec[t], ws.th_f[t], ws.th_b[t], ws.ss[t], ws.scale[t], ws.shift[t],
                    ws.zprob[t], ws.zmask[t], ws.zval[t], ws.zc[t])
            _ops.asr_step_forward_(B, t, self.train, fix, thr, temp, float(self.scale_prior_mean),
                                   float(self.scale_prior_variance), self.scale_prior_log_variance,
                                   float(self.hyper("constrains_num_gamma")), w20,
                                   gw8 if learned else [], hid_l, *outs)
            if self.live_hook is not None:
                self.live_hook(ws.live, t)
            if self.fused_step:
                self._step_fused(X, ws, t, lik_std)
                continue
            if self._f32_parts(B):
                self._vae_forward_all(X, ws, lik_std, t, t + 1, save=need_grad)
                continue
            self._vae_encoder(X, ws, t, t + 1, ws.runloss)
            if defer:
                continue  # only z feeds the recurrence: the generative half waits
            self._vae_decoder(ws, lik_std, t, t + 1)
            ops.stn_forward(ws.r[t], ws.th_b[t], (C, C), out=ws.canvas, z=ws.zval[t],
                            mask=ws.zmask[t], accumulate=True)
        if defer and not self._f32_parts(B):
            # the decoder of every step over T*B rows in one set of launches,
            # then the canvas accumulated in step order (the same bits)
            self._vae_decoder(ws, lik_std, 0, T)
            for t in range(T):
                ops.stn_forward(ws.r[t], ws.th_b[t], (C, C), out=ws.canvas, z=ws.zval[t],
                                mask=ws.zmask[t], accumulate=True)
        self._forward_loss(X, targets, ws, need_grad, outputs)

    # fp32 below FUSED_F32_MIN_ROWS: the generative half of each step's VAE
    # (which feeds only the canvas, never the loop) after the loop, over T*B
    # rows (DEFER_DECODER = False: inside the loop, step by step)
    DEFER_DECODER = True

    def _forward_loss(self, X, targets, ws, need_grad, outputs=True):
        """elbo (:917-935, recon :937-962) + pr_loss + element + margin
        (:964-1079)."""
        B, T, C2 = ws.B, self.max_steps, self.C2
        g = self._gammas()
        _ops.asr_terms_(B, T, self.canvas_size, self._cons, g, ws.arec, ws.vkl, ws.zmask, ws.live,
                        ws.klsum, ws.pr, ws.area, ws.outl, ws.size, ws.over, ws.zsum)
        if self.zsum_hook is not None:
            self.zsum_hook(ws.zsum)
        parts = ws.cparts
        self._loss_inputs = (X, targets)
        ws.materialized = bool(outputs)
        gscale = self._gscale(B)
        _ops.recon_loss_(X, ws.canvas if (outputs or parts is None) else None, parts,
                         T if parts is not None else 0, B * C2, ws.prows, self.canvas_size,
                         ws.klsum, ws.digits, targets, B, C2, float(gscale),
                         ws.recon if outputs else None, ws.bce, ws.mse, ws.loss_b,
                         ws.acc_b if targets is not None else None,
                         ws.dcanvas if need_grad else None)
        _ops.asr_finalize_(B, T, self.canvas_size, self._cons, g, float(self._gscale(B)), ws.arec,
                           ws.live, ws.zsum, ws.pr, ws.loss_b, ws.element, ws.margin)
        _ops.batch_mean_(ws.loss_b, ws.acc_b if targets is not None else None, ws.mse, None, B,
                         ws.means)
        _ops.add_(ws.means, ws.margin, ws.means, 1)
        self._outputs_ready = True

    # --------------------------------------------------------- backward ---
    def _backward(self, X, ws):
        self._backward_body_grouped(X, ws)  # (the body zeroes its own accumulators)

    def _backward_body(self, X, ws):
        B, T, H, Z = ws.B, self.max_steps, self.rnn_units, self.vae_latent_dimensions
        W, C2 = self.windows_size, self.C2
        # the gradient buffer and the LSTM chains' accumulators in one launch
        _ops.fill32_batch_([self.params.grad, ws.dh, ws.dhg, ws.dGsum, ws.dGgsum], [0] * 5)
        Ki = self._Kpad("infer_rnn_running/kernel")
        Kg = self._Kpad("gen_rnn_running/kernel")
        gscale = self._gscale(B)
        fix = self._fix
        w20 = self._w20()
        _ops.asr_terms_backward_(B, T, self.canvas_size, self._cons, self._gammas(), float(gscale),
                                 float(gscale), ws.arec, ws.live, ws.zsum, ws.dreg)
        head_w = [self._P(n + "/kernel")[:H] for n in ("inf_shift/dense", "inf_shift/dense_2",
                                                     "z_pres/log_odds/dense", "inf_scale/dense",
                                                     "inf_scale/dense_2")]
        gen_w = [self._P(n + "/kernel") for n in ("gen_shift/dense", "gen_shift/dense_2")]
        learned = not self.fix_scale_distribution
        nh = self._nhid
        gen_k = (3, 4, 8, 9) if learned else (3, 4)
        if learned:
            # the gen_scale hidden layers read hg_t too: the same chain into dhg[t]
            gen_w += [self._P("gen_scale/dense/kernel")[:H], self._P("gen_scale/dense_2/kernel")[:H]]
            gw8 = self._gw8()
        steps_side = (self.VAE_WGRAD_PER_STEP and self.grad_reducer is None
                      and B >= self.SIDE_MIN_BATCH)
        side = self._side_stream() if steps_side else None
        ws.vae_wgrads_done = steps_side
        ws.u_wgrads_done = steps_side and self.U_WGRAD_PER_STEP
        # every step's STN write backward in ONE launch over T*B rows, before
        # the loop (it reads only the forward's records and the canvas
        # gradient, shared by the steps; the AIR model's _backward_body does
        # the same): six launches of B rows -> one
        self._stn_write_backward_all(ws)
        # and the decoder half of every step's VAE backward (dz_t before the
        # loop's carry), likewise over T*B rows; the reversed loop runs only
        # the encoder half per step
        self._vae_decoder_backward(ws, 0, T)
        # a small batch's recurrent-input gradient in DH_PARTS K slices
        # (_dh_parts: the serial K = 4H chain per workgroup cut)
        parts = self._dh_parts(B)
        if parts:
            dUp, dUgp = ws.buffer("dUp", (parts, B, LU)), ws.buffer("dUgp", (parts, B, LU))
        for t in reversed(range(T)):
            self._vae_encoder_backward(ws, t, t + 1, gscale)
            if steps_side:
                # step t's VAE weight gradients are final: accumulate them on
                # the side stream under the rest of the loop
                with torch.cuda.stream(self._fork(side)):
                    self._vae_weight_grads(ws, t)
            ops.stn_backward(X, ws.th_f[t], (W, W), ws.dg_all[t], want_dU=False, dtheta=ws.dth_f)
            hid = [ws.hid8[k, t] for k in range(nh)]
            dpre = [ws.dpre[k, t] for k in range(nh)]
            tail = ([x if (k != 5 or fix < 0) else None for k, x in enumerate(hid)],
                    ws.arec[t], ws.eps_shift[t], ws.eps_scale[t], ws.dth_f, ws.dth_b_all[t],
                    ws.dot_all[t], ws.dreg[t], ws.dss_carry if t < T - 1 else None, ws.douts[t],
                    [x if (k != 5 or fix < 0) else None for k, x in enumerate(dpre)])
            _ops.asr_step_backward_(B, self.train, fix, float(self.hyper("z_pres_temperature")),
                                    float(self.scale_prior_mean),
                                    float(self.scale_prior_variance), float(gscale), w20,
                                    gw8 if learned else [], *tail)
            # dh[t] += the five heads reading h_t; dhg[t] += the generative shift
            # heads; dhg[t-1] += the prior at step t (it reads hg_{t-1}): three
            # chains of one shape in one launch
            probs = [([dpre[k] for k in (0, 1, 2, 6, 7)], head_w, ws.dh[t], ws.dh[t]),
                     ([dpre[k] for k in gen_k], gen_w, ws.dhg[t], ws.dhg[t])]
            if fix < 0 and t > 0:
                probs.append(([dpre[5]], [self._P("z_pres/prior/dense/kernel")], ws.dhg[t - 1],
                              ws.dhg[t - 1]))
            if learned:
                # 5 + 4 + 1 segments pass the launch's eight: dhg[t]'s chain on its own
                ops.gemm_kseg_group(probs[1:2], B, H, 64, 64, 64, H, transB=True)
                del probs[1]
            ops.gemm_kseg_group(probs, B, H, 64, 64, 64, H, transB=True)
            dc_in = ws.dc[(t + 1) % 2] if t < T - 1 else None
            dcg_in = ws.dcg[(t + 1) % 2] if t < T - 1 else None
            # (both cells in one launch)
            _ops.lstm_cell_backward2_(ws.G[t], ws.c[t - 1] if t > 0 else None, ws.c[t], ws.dh[t],
                                      dc_in, ws.dG[t], ws.dc[t % 2], ws.dGsum, ws.Gg[t],
                                      ws.cg[t - 1] if t > 0 else None, ws.cg[t], ws.dhg[t],
                                      dcg_in, ws.dGg[t], ws.dcg[t % 2], ws.dGgsum, B, H)
            if steps_side and self.U_WGRAD_PER_STEP:
                # step t's recurrent-rows gradients likewise (dG_t, dGg_t final)
                with torch.cuda.stream(self._fork(side)):
                    self._u_rows_wgrad(ws, t)
            if t > 0 and parts:
                # a small batch: the same product in `parts` K slices (one batched
                # launch of 2 x parts), summed in part order by the unpack
                kp = 4 * H // parts
                gemm([ws.dG[t][:, j * kp:] for j in range(parts)]
                     + [ws.dGg[t][:, j * kp:] for j in range(parts)],
                     [Ki[C2:][:, j * kp:] for j in range(parts)]
                     + [Kg[:, j * kp:] for j in range(parts)],
                     [dUp[j] for j in range(parts)] + [dUgp[j] for j in range(parts)],
                     B, LU, kp, 4 * H, 4 * H, LU, transB=True)
                _ops.asr_unpack_parts_(B, Z, H, LU, dUp, dUgp, parts, ws.dz_all[t - 1],
                                       ws.dss_carry, ws.dh[t - 1], ws.dhg[t - 1], 1)
            elif t > 0:
                # N = LU: the 3 pad columns of dU / dUg are scratch (unpack skips them)
                # (both LSTMCells in one batched launch: same shapes and chains)
                gemm([ws.dG[t], ws.dGg[t]], [Ki[C2:], Kg], [ws.dU, ws.dUg], B, LU, 4 * H,
                     4 * H, 4 * H, LU, transB=True)
                # the latent carry added straight into step t-1's dz (its decoder
                # half is there already: no separate add launch)
                _ops.asr_unpack_(B, Z, H, LU, ws.dU, ws.dUg, ws.dz_all[t - 1], ws.dss_carry,
                                 ws.dh[t - 1], ws.dhg[t - 1], 1)
        self._weight_grads(X, ws)
        if steps_side:
            torch.cuda.current_stream().wait_stream(side)
        self._reduce_bucket(0, self.params.total)

    def _u_rows_wgrad(self, ws, t):
        """The LSTMCells' recurrent-rows kernel gradients U^T dG (all T*B rows,
        or loop step t's B rows, accumulated)."""
        B, T, H = ws.B, self.max_steps, self.rnn_units
        K = B if t is not None else B * T
        v = _step_rows(T, t)
        gKi = self._Kpad("infer_rnn_running/kernel", "grad")
        gKg = self._Kpad("gen_rnn_running/kernel", "grad")
        # tall (plan_wgrads): both cells in one grouped x3 launch, as AIR's
        # recurrent rows: 312 x 1024 x K each, deterministic
        self._wgrads([WgradProblem(v(ws.U), v(ws.dG), gKi[self.C2:], None, LU, 4 * H, LU, 4 * H),
                      WgradProblem(v(ws.Ug), v(ws.dGg), gKg, self._G("gen_rnn_running/bias"),
                                   LU, 4 * H, LU, 4 * H)],
                     K, "rec_wgrad_x3", tall=self.REC_WGRAD_X3, check_even=False)

    # (with VAE_WGRAD_PER_STEP) the recurrent-rows gradients per step too (9.20 ->
    # 8.96 ms; the heads' gradients per step as well measured neutral, 9.01 vs
    # 9.26 ms for neither on a slower box, and stay after the loop)
    U_WGRAD_PER_STEP = True

    # one GPU, from SIDE_MIN_BATCH: the VAE weight gradients of loop step
    # t accumulate on the side stream as soon as that step's VAE backward is
    # done, under the latency-bound rest of the reversed loop, instead of over
    # all T*B rows after it (VAE_WGRAD_PER_STEP = False: after the loop)
    VAE_WGRAD_PER_STEP = True

    def _weight_grads(self, X, ws):
        B, H, C2 = ws.B, self.rnn_units, self.C2
        heads_s3 = ws.vae_wgrads_done and self.HEADS_S3
        if heads_s3:
            # the heads' weight gradients on the third stream, beside the
            # x-rows gradient (main) and step 0's on the side stream
            with torch.cuda.stream(self._fork(self._stream3())):
                self._heads_wgrad(ws, None)
        if not ws.vae_wgrads_done:  # (else per loop step, on the side stream)
            self._vae_weight_grads(ws)
        ws.vae_wgrads_done = False
        # LSTMCells: x rows from sum_t dG (the x input is loop-invariant)
        x3p = ws.x3_ready is not None
        if x3p:
            # the AIR x-rows gradient's pre-split form: X's pieces from the
            # forward's side stream, dGsum's split here
            torch.cuda.current_stream().wait_event(ws.x3_ready)
            ws.x3_ready = None
            ops.split3_bf16(ws.dGsum, ws.buffer("dG3", (3, B, 4 * H), torch.bfloat16), B, 4 * H,
                            4 * H, 4 * H, B * 4 * H)
        self._x_rows_grad(X, ws, self._Kpad("infer_rnn_running/kernel", "grad"),
                          self._G("infer_rnn_running/bias"), 0, C2, x3p)
        # M = LU (16-byte aligned LDS-DMA operands): rows Z+3+H.. of the
        # product land in the kernels' own pad rows (ParamStore pad), never in
        # a neighbouring variable's gradient
        if not ws.u_wgrads_done:
            self._u_rows_wgrad(ws, None)
        ws.u_wgrads_done = False
        if heads_s3:
            torch.cuda.current_stream().wait_stream(self._stream3())
        else:
            self._heads_wgrad(ws, None)

    # (with the per-step gradients) the heads' gradients on the third stream
    HEADS_S3 = True

    def _heads_wgrad(self, ws, t):
        """The heads' weight gradients (all T*B rows, or loop step t's B rows,
        accumulated)."""
        B, T, H, Z = ws.B, self.max_steps, self.rnn_units, self.vae_latent_dimensions
        K = B if t is not None else B * T
        v = _step_rows(T, t)
        G = self._G
        P = WgradProblem

        def hidden(X, lda, layers):
            """[H x 64] hidden layers reading X, one batched launch: (layer, its dpre)"""
            self._wgrads([P(X, v(ws.dpre[k]), G(n + "/kernel")[:H], G(n + "/bias"), H, 64, lda, 64)
                          for n, k in layers], K)
        # (the learned scale prior's layers sit beside gen_shift's and inf_scale's)
        gen_scale = [] if self.fix_scale_distribution else [("gen_scale/dense", 8),
                                                            ("gen_scale/dense_2", 9)]
        inf_scale = [("inf_scale/dense", 6), ("inf_scale/dense_2", 7)]
        hidden(v(ws.h), H, [("inf_shift/dense", 0), ("inf_shift/dense_2", 1),
                            ("z_pres/log_odds/dense", 2)] + inf_scale)
        hidden(v(ws.hg), H, [("gen_shift/dense", 3), ("gen_shift/dense_2", 4)] + gen_scale)
        if self._fix < 0:  # (the prior reads hg_{t-1}, inside Ug)
            hidden(v(ws.Ug)[..., Z + 3:], LU, [("z_pres/prior/dense", 5)])
        # the shift-latent rows of the scale hidden layers
        self._wgrads([P(v(ws.ss), v(ws.dpre[k]), G(n + "/kernel")[H:], None, 2, 64, 3, 64)
                      for n, k in inf_scale + gen_scale], K)
        # output layers from douts [T, B, 12] ([T, B, 14] with the learned
        # scale prior): (layer, its hidden activation, its douts column)
        d, dn = v(ws.douts), self._dn
        two = [("inf_shift/dense_1", 0, 0), ("inf_shift/dense_3", 1, 2),
               ("gen_shift/dense_1", 3, 5), ("gen_shift/dense_3", 4, 7)]
        one = [("z_pres/log_odds/dense_1", 2, 4)] + (
            [("z_pres/prior/dense_1", 5, 9)] if self._fix < 0 else [])
        scl = [("inf_scale/dense_1", 6, 10), ("inf_scale/dense_3", 7, 11)]
        if gen_scale:
            scl += [("gen_scale/dense_1", 8, 12), ("gen_scale/dense_3", 9, 13)]

        def out(n, h, c, k):
            """a [64 x k] output layer; its kernel's first 64 rows are all of
            it, but for scl's, which have two more for the shift latent"""
            return P(v(ws.hid8[h]), d[..., c:], G(n + "/kernel")[:64], G(n + "/bias"), 64, k, 64, dn)
        # one batched launch per shape (each is a tiny [64 x 1..2] product
        # over K = T*B rows: launch-bound one by one)
        self._wgrads([out(*l, 2) for l in two] + [out(*l, 1) for l in one + scl], K)
        self._wgrads([P(v(ws.ss), d[..., col:], G(n + "/kernel")[64:], None, 2, 1, 3, dn)
                      for n, _, col in scl], K)

    # ------------------------------------------------------- outputs -----
    def _records(self, name):
        return self._bt(self._ws.arec[:, Q[name]])

    @property
    def z_pres_kls(self):
        return self._records("zkl")

    @property
    def scale_kls(self):
        return self._records("skl")

    @property
    def shift_kls(self):
        return self._records("shkl")

    @property
    def vae_kls(self):
        ws = self._ws
        return self._bt(ws.vkl * ws.zmask)

    @property
    def log_variables(self) -> Dict[str, float]:
        """Batch means of the reference's log_variables (:1080-1084)."""
        ws = self._ws
        T = self._T()
        m = lambda v: float(v.mean())  # noqa: E731
        kls = {k: float(self._records(k).sum(1).mean()) for k in ("zkl", "skl", "shkl")}
        return {"z_pres_kl": kls["zkl"], "scale_kl": kls["skl"], "shift_kl": kls["shkl"],
                "vae_kl": float((ws.vkl * ws.zmask)[:T].sum(0).mean()),
                "pr_num": float(self._records("prn").sum(1).mean()),
                "recon": m(ws.bce), "mse": m(ws.mse), "area_loss": m(ws.area),
                "out_loss": m(ws.outl), "size_loss": m(ws.size), "over_loss": m(ws.over),
                "num_margin": float(ws.margin[0]), "num_min_KL": m(ws.element),
                "TotLoss": self.loss, "elbo": m(ws.klsum + ws.bce), "accu": self.accuracy}

    log_names = ops.ASR_LOG_NAMES  # the keys of ``log_variables``, in its order

    def log_row_(self, out: torch.Tensor) -> None:
        """``log_variables`` of the last step (or infer) into the device fp32
        vector ``out`` [16] on the current stream: one launch
        (ops.asr_log_row), no host read.  The sums run in float64 on the
        device, so an entry may differ from the property's fp32 reduction by
        that reduction's rounding; TotLoss, accu and num_margin are its bits."""
        ws = self._log_row_out(out)
        ops.asr_log_row(ws.arec, ws.vkl, ws.zmask, ws.live, ws.bce, ws.mse, ws.area, ws.outl,
                        ws.size, ws.over, ws.element, ws.klsum, ws.margin, ws.means, out,
                        slots=[Q[n] for n in ("zkl", "skl", "shkl", "prn")])

    # ------------------------------------------------------ generation -----
    _GEN_NOISE = (("eps_shift", True), ("eps_scale", True), ("eps_z", True), ("eps_x", True),
                  ("u_x", False), ("u", False))

    def generate(self, batch=None, noise=None):
        """The test model's ``generated_samples``
        (air_number_bbox_location.py:1124-1361, vae.py:51-86): up to
        ``max_steps`` objects per canvas.  Each step runs the generative
        LSTMCell on [z_prev, latents_prev], draws the shift latent from the
        gen_shift heads, the scale latent from the scale prior (the constant
        one, or the gen_scale heads on [output, shift latent] with
        ``fix_scale_distribution=False``) and z from the VAE prior, decodes and binarises the window
        (``sample_from_mean``), and writes it where the rounded z_pres sample
        (fixed +-100 prior with ``fix_steps``, else the learned prior on the
        previous generative output) keeps the image counting.  The write
        scale is the constant mean(constrains_area_minmax) / canvas_size
        (:1203-1205); where that mean is not positive the reference builds
        infinite transforms, and this raises ``ValueError`` instead.

        Returns the canvas [G, C, C, 1]; ``generated_st_back`` [G, T_exec, 2,
        3] and ``generated_num_digits`` [G] hold the loop's other outputs.
        ``noise`` (optional) injects eps_shift [T,G,2], eps_scale [T,G], eps_z
        [T,G,Z], eps_x [T,G,W2], u_x [T,G,W2], u [T,G] (T = max_steps);
        otherwise device Philox noise is drawn in that order.  The loop runs
        max_steps iterations on the device without a host synchronisation
        (steps past the reference's exit write nothing); the executed count is
        read back once at the end.  Runs the fp32 GEMMs in either precision."""
        G = int(batch if batch is not None else self.generation_batch_size)
        T, C, W2, Z, H = self.max_steps, self.canvas_size, self.W2, self.vae_latent_dimensions, \
            self.rnn_units
        area = sum(self.constrains_area_minmax) / len(self.constrains_area_minmax)
        if not area > 0:
            raise ValueError("generation writes at the scale mean(constrains_area_minmax) / "
                             f"canvas_size, which must be positive (got {area / C})")
        s = torch.tensor(area / C, dtype=torch.float32).item()  # one cast of the double quotient
        G1, G2 = self.vae_generative_units
        dev = self.device
        e = lambda *sh: torch.empty(sh, device=dev, dtype=torch.float32)  # noqa: E731
        eps = {"eps_shift": e(T, G, 2), "eps_scale": e(T, G), "eps_z": e(T, G, Z),
               "eps_x": e(T, G, W2), "u_x": e(T, G, W2), "u": e(T, G)}
        for k, normal in self._GEN_NOISE:
            buf = eps[k]
            if noise is not None:
                src = torch.as_tensor(noise[k], dtype=torch.float32)
                if tuple(src.shape) != tuple(buf.shape):
                    raise ValueError(f"noise[{k}] has shape {tuple(src.shape)}, expected "
                                     f"{tuple(buf.shape)}")
                buf.copy_(src)
            else:
                ops.rng_fill(buf, self.noise_seed, self._noise_ctr, normal)
                self._noise_ctr += (buf.numel() + 3) // 4
        canvas, stop = e(G, C * C), e(G)
        digits = torch.empty(G, device=dev, dtype=torch.int32)
        live = torch.empty(T + 1, device=dev, dtype=torch.int32)
        hg_zero = e(G, H)
        _ops.fill32_batch_([canvas, stop, digits, live[:1], live[1:], hg_zero], [0, 0, 0, 1, 0, 0])
        Ug, Gg, cg, hg = e(G, LU), e(G, 4 * H), e(2, G, H), e(2, G, H)
        hid = e(3, G, 64)
        ss, z, st_back = e(2, G, 3), e(2, G, Z), e(T, G, 6)
        zval, zmask = e(G), e(G)
        d1, d2, r, win = e(G, G1), e(G, G2), e(G, W2), e(G, W2)
        Kg, bg = self._Kpad("gen_rnn_running/kernel"), self._P("gen_rnn_running/bias")
        fix = self._fix
        heads = ["gen_shift/dense", "gen_shift/dense_2"] + (["z_pres/prior/dense"] if fix < 0 else [])
        relu_w = [self._P(n + "/kernel") for n in heads]
        relu_b = [self._P(n + "/bias") for n in heads]
        outs = ("gen_shift/dense_1", "gen_shift/dense_3", "z_pres/prior/dense_1")
        w6 = [self._P(n + p) for n in outs for p in ("/kernel", "/bias")]
        vw = {n: self._P("vae/" + n + "/weights") for n in ("generative_1", "generative_2",
                                                            "gen_mean")}
        vb = {n: self._P("vae/" + n + "/biases") for n in vw}
        thr, temp = self.hyper("stopping_threshold"), self.hyper("z_pres_temperature")
        lik_std = float(self.hyper("vae_likelihood_std"))
        learned = not self.fix_scale_distribution
        if learned:
            ghid = e(2, G, 64)
            gw8 = self._gw8()
            gsc_w = [gw8[0][:H], gw8[4][:H]]
        for t in range(T):
            cur, prv = t % 2, (t - 1) % 2
            prev = t > 0
            _ops.asr_pack_(G, Z, H, LU, z[prv] if prev else None, ss[prv] if prev else None,
                           hg[prv] if prev else None, Ug, None, None)
            # K = LU: the packed rows and the kernel's pad rows end in zeros (_forward)
            gemm([Ug], [Kg], [Gg], G, 4 * H, LU, LU, 4 * H, 4 * H, bias=[bg])
            _ops.lstm_cell_forward_(Gg, None, cg[prv] if prev else None, cg[cur], hg[cur], G, H)
            # the gen_shift hidden layers on the new output and the learned
            # prior's on the previous one (:1259-1272), one batched launch
            ra = [hg[cur]] * 2 + ([hg[prv] if prev else hg_zero] if fix < 0 else [])
            gemm(ra, relu_w, [hid[k] for k in range(len(ra))], G, 64, H, H, 64, 64, epi=EPI_RELU,
                 bias=relu_b)
            hid3 = [hid[0], hid[1], hid[2] if fix < 0 else None]
            tail = (eps["eps_shift"][t], eps["eps_scale"][t], eps["eps_z"][t], eps["u"][t], stop,
                    digits, live, ss[cur], z[cur], st_back[t], zval, zmask)
            if learned:
                # the gen_scale hidden layers' chains over the new output (the
                # kernel adds the shift latent's terms, bias and relu)
                gemm([hg[cur]] * 2, gsc_w, [ghid[0], ghid[1]], G, 64, H, H, 64, 64, epi=EPI_STORE)
            _ops.asr_gen_step_(G, Z, t, fix, thr, temp, float(self.scale_prior_mean),
                               float(self.scale_prior_variance), s, float(self.vae_prior_mean),
                               self.vae_prior_log_variance, w6, hid3, gw8 if learned else [],
                               [ghid[0], ghid[1]] if learned else [], *tail)
            gemm([z[cur]], [vw["generative_1"]], [d1], G, G1, Z, Z, G1, G1, epi=EPI_SOFTPLUS,
                 bias=[vb["generative_1"]])
            gemm([d1], [vw["generative_2"]], [d2], G, G2, G1, G1, G2, G2, epi=EPI_SOFTPLUS,
                 bias=[vb["generative_2"]])
            gemm([d2], [vw["gen_mean"]], [r], G, W2, G2, G2, W2, W2, epi=EPI_SIGMOID_NOISE,
                 bias=[vb["gen_mean"]], aux=[eps["eps_x"][t]], ldaux=W2, aux_scale=lik_std)
            _ops.bernoulli_threshold_(r, eps["u_x"][t], win, G * W2)
            ops.stn_forward(win, st_back[t], (C, C), out=canvas, z=zval, mask=zmask,
                            accumulate=True)
        Tx = int(live[:T].sum().item())  # the one readback: the reference's executed steps
        self.generated_st_back = st_back[:Tx].transpose(0, 1).reshape(G, Tx, 2, 3)
        self.generated_num_digits = digits
        self.generated_samples = canvas.reshape(G, C, C, 1)
        return self.generated_samples
