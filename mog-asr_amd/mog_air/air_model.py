"""AIRModel — drop-in host object for the reference's AIR baseline model
(air/air_model.py:13-1146), running the per-object-step loop on MI355X HIP
kernels (libmog_air.so) with a hand-scheduled forward and backward.  The part
it shares with the AIR-ASR model (constructor, workspace, streams, noise, the
public API) is ModelBase (model_base.py); this file is the AIR loop.

Reference surface kept (air_model.py:15-51, training_air_original.py:158-209):
the constructor keyword arguments, variable sharing between a train model and
a test model (``reuse``), annealing schedules (air_model.py:139-147,164-184)
and the result attributes ``loss, accuracy, mse_loss, global_step,
rec_num_digits, rec_scales, rec_shifts, rec_st_back, rec_windows, rec_latents,
reconstruction, reconstruction_loss, z_pres_probs, z_pres_kls, scale_kls,
shift_kls, vae_kls, accuracy_instance``.  TF's ``sess.run([model.training,
...])`` becomes ``model.step(images, targets)``; fetching the test model's
tensors becomes ``model.infer(images, targets)``.

Loop semantics: the data-dependent ``tf.while_loop`` (air_model.py:428-432)
runs max_steps iterations on the device with the predicate folded into a
per-step ``live`` flag; every loss term, count and gradient is identical to
the early exit, and the ``rec_*`` outputs are sliced to the executed steps.
No host synchronisation happens inside a train step.

``cnn=True`` (the reference default, air_model.py:763-810): the LSTM reads the
1152 features of a three-convolution encoder (csrc/cnn_enc.hip) instead of
the canvas; fp32, one device, ``cnn_filters=8``, 50 x 50 canvases (DESIGN.md
§4.14).  ``rnn_input`` holds them after a forward.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import numpy as np
import torch

from . import ops
from .model_base import R_NREC, ModelBase, _Workspace, annealed_value  # noqa: F401
from .ops import EPI_RELU, gemm
from .params import CNN_LAYERS, cnn_param_specs, param_specs
from .results import Generation
from .wgrads import TALL_X3, WgradProblem

_ops = ops._ops  # torch.ops.mog_air (csrc/torch_ops.cpp)

# step-record slots (air_cell.hip enum; R_NREC of them)
R_SM, R_SLV, R_HM0, R_HM1, R_HLV0, R_HLV1, R_LO, R_S, R_TX, R_TY, R_Y, R_Z = range(12)
R_ACT_OLD, R_ACT, R_LIVE, R_ZC, R_ZTERM = 12, 13, 14, 15, 16


def marginal_objective(num_prior, max_steps) -> np.ndarray:
    """The ``-ap`` per-step prior bias (air_model.py:86-107)."""
    obj = np.zeros([max_steps])
    buf = 1.0 - 1.0 / len(num_prior)
    for ind in range(max_steps):
        if ind not in num_prior and ind < max(num_prior):
            obj[ind] = 1.0
        else:
            if ind == max(num_prior):
                break
            obj[ind] = buf
            if ind in num_prior:
                buf -= 1.0 / len(num_prior)
    for ind in range(max_steps):
        if obj[ind] == 1.0:
            obj[ind] = 100
        elif obj[ind] == 0.0:
            obj[ind] = -100.0
        else:
            obj[ind] = np.log(obj[ind] / (1.0 - obj[ind]))
    return obj.astype(np.float32)


class AIRModel(ModelBase, Generation):
    """See module docstring.  Extra keyword-only arguments (not in the
    reference): ``device``, ``seed`` (weight init), ``noise_seed`` (device
    Philox noise), ``grad_world`` (data-parallel world size folded into the
    loss-mean gradient scale)."""

    def __init__(self, input_images=None, target_num_digits=None, max_steps=3, max_digits=2,
                 rnn_units=256, canvas_size=50, windows_size=28, vae_latent_dimensions=50,
                 vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                 scale_prior_mean=-1.0, scale_prior_variance=0.1, shift_prior_mean=0.0,
                 shift_prior_variance=1.0, vae_prior_mean=0.0, vae_prior_variance=1.0,
                 vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64,
                 z_pres_hidden_units=64, z_pres_prior_log_odds=-2.0, z_pres_temperature=1.0,
                 stopping_threshold=0.99, learning_rate=1e-3, gradient_clipping_norm=100.0,
                 cnn=True, cnn_filters=8, num_summary_images=60, train=False, reuse=False,
                 scope="air", annealing_schedules=None, generation_batch_size=64,
                 num_prior=None, *, device=None, seed: int = 1235, noise_seed: int = 1235,
                 grad_world: int = 1, precision: str = "fp32", fused_step: bool = True,
                 batch_vae: bool = True):
        if cnn:
            # the reference hard-codes the 50 x 50 canvas and the 12 x 12 plane
            # it flattens (air_model.py:763-810)
            if canvas_size != ops.CNN_CANVAS:
                raise ValueError(f"cnn=True reads a {ops.CNN_CANVAS} x {ops.CNN_CANVAS} canvas "
                                 f"(air_model.py:763-810), got canvas_size={canvas_size}")
            if cnn_filters != 8:
                raise NotImplementedError(
                    "cnn=True is built for cnn_filters=8 (the reference default), got "
                    f"{cnn_filters}")
            if precision != "fp32":
                raise NotImplementedError(
                    "cnn=True runs in fp32 only; the bf16 configuration of the encoder is a "
                    "follow-up")
        if not (scale_hidden_units == shift_hidden_units == z_pres_hidden_units):
            raise NotImplementedError("heads must share one hidden width")
        super().__init__(
            input_images=input_images, target_num_digits=target_num_digits, max_steps=max_steps,
            max_digits=max_digits, rnn_units=rnn_units, canvas_size=canvas_size,
            windows_size=windows_size, vae_latent_dimensions=vae_latent_dimensions,
            vae_recognition_units=vae_recognition_units, vae_generative_units=vae_generative_units,
            scale_prior_mean=scale_prior_mean, scale_prior_variance=scale_prior_variance,
            shift_prior_mean=shift_prior_mean, shift_prior_variance=shift_prior_variance,
            vae_prior_mean=vae_prior_mean, vae_prior_variance=vae_prior_variance,
            vae_likelihood_std=vae_likelihood_std, scale_hidden_units=scale_hidden_units,
            shift_hidden_units=shift_hidden_units, z_pres_hidden_units=z_pres_hidden_units,
            z_pres_prior_log_odds=z_pres_prior_log_odds, z_pres_temperature=z_pres_temperature,
            stopping_threshold=stopping_threshold, learning_rate=learning_rate,
            gradient_clipping_norm=gradient_clipping_norm, num_summary_images=num_summary_images,
            train=train, scope=scope, annealing_schedules=annealing_schedules,
            generation_batch_size=generation_batch_size, device=device, noise_seed=noise_seed,
            grad_world=grad_world, precision=precision, fused_step=fused_step)
        # the glimpse VAE of all T steps after the loop, over T*B rows.
        # (Measured and not kept: step 0's VAE on a second stream under the
        # rest of the recurrent loop -- no gain at B = 8192, slower at 64.)
        self.batch_vae = bool(batch_vae)
        self.num_prior = num_prior
        if num_prior is not None:
            self.marginal = marginal_objective(num_prior, self.max_steps)
        # cnn=True: the LSTM reads the conv encoder's 12 x 12 x F features
        # instead of the canvas (air_model.py:763-810); the image still feeds
        # the STN read and the reconstruction loss
        self.cnn, self.cnn_filters = bool(cnn), int(cnn_filters)
        if self.cnn:
            self.lstm_in = ops.CNN_POOL2 ** 2 * self.cnn_filters
        specs = param_specs(
            self.lstm_in, self.rnn_units, self.W2, self.vae_recognition_units,
            self.vae_generative_units, self.vae_latent_dimensions, scale_hidden_units,
            z_pres_hidden_units)
        if self.cnn:  # appended: every other variable keeps its offset and draw
            specs += cnn_param_specs(self.cnn_filters)
        self._bind_params(scope, specs, reuse, seed)

    _HEADS = ("scale/mean", "scale/log_variance", "shift/mean", "shift/log_variance",
              "z_pres/log_odds")

    def _bucket_split(self) -> int:
        """Flat offset where the glimpse-side variables (heads, VAE) start:
        [0, split) is the LSTM kernel + bias, [split, total) everything else
        (params.param_specs order; cnn=True appends the encoder's there)."""
        return self.params.offsets[self._SCOPE_PREFIX + "scale/mean/hidden/weights"]

    # ------------------------------------------------ cnn=True encoder ---
    def _cnn_tensors(self, buf: str = "flat"):
        """(w1, b1, w2, b2, w3, b3) of the encoder in the parameter (or
        gradient) buffer."""
        return [self.params.view("air/cnn/" + layer + "/" + n, buf)
                for layer in CNN_LAYERS for n in ("kernel", "bias")]

    def _cnn_forward(self, X, ws):
        """conv1 -> pool -> conv2 -> pool -> conv3 in one launch
        (csrc/cnn_enc.hip); returns the features [B, 144 F], the LSTM's input."""
        if self.grad_reducer is not None or self.live_hook is not None:
            raise NotImplementedError(
                "cnn=True is the single-device step; data parallelism (a grad_reducer or "
                "live_hook attached) is a follow-up")
        with self._timed("cnn_enc_forward"):
            ops.cnn_enc_forward(X, self._cnn_tensors(), ws.pool1, ws.pool2, ws.feat)
        return ws.feat

    @property
    def rnn_input(self):
        """The LSTM input of the last forward (the reference's attribute):
        the encoder's features [B, 144 F] (cnn=True) or the flat canvas."""
        if self._ws is None or not self._outputs_ready:
            raise RuntimeError("rnn_input: no forward has run")
        return self._ws.feat if self.cnn else self._loss_inputs[0]

    # batched VAE: every step's heads and scalars in one launch each after
    # the LSTM chain (False: per step, as the unbatched loop;
    # tests/test_gpu_steps_fwd.py compares the two bitwise)
    STEPS_ONE_LAUNCH = True

    # ----------------------------------------------------------- forward ---
    def _forward(self, X: torch.Tensor, targets: Optional[torch.Tensor], ws: _Workspace,
                 need_grad: bool, outputs: bool = True) -> None:
        B, T, H = ws.B, self.max_steps, self.rnn_units
        C, W, C2, W2 = self.canvas_size, self.windows_size, self.C2, self.W2
        HS = self.scale_hidden_units
        K = self._P("rnn/basic_lstm_cell/kernel")
        bK = self._P("rnn/basic_lstm_cell/bias")
        NX = self.lstm_in
        Wx, Wh = K[:NX], K[NX:]
        # the LSTM's input: the canvas, or the encoder's features (main
        # stream, ahead of everything that reads them)
        Xl = self._cnn_forward(X, ws) if self.cnn else X
        side = self._side_stream() if ws.noise_side else None
        ws.noise_side = False
        if self.cnn and need_grad and self._x3p_xgrad(B):
            self._x_split3(Xl, ws)  # (main stream: the features are made there)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            # (after the noise on the side stream, when it went there)
            self._reset_loop_state(ws)
            if need_grad and self._x3p_xgrad(B) and not self.cnn:
                self._x_split3(X, ws)  # the x-part gradient's A operand, split once per step
            if need_grad and self.precision == "bf16":
                self._x_bf16(X, ws)  # (likewise: the bf16 x-part gradient's A operand)
            if (need_grad and self.precision == "fp32" and self.VAE_DX_X3
                    and B * self.max_steps >= self.X3_DX_MIN_ROWS):
                # the x3 input gradients' weight pieces, split here instead of
                # on the backward's path (fp32 step 3.05 -> 3.02 ms)
                self._w3()
            if side is not None:
                pre_done = torch.cuda.Event()
                pre_done.record(side)
        prior_lo = self.hyper("z_pres_prior_log_odds")
        temperature = self.hyper("z_pres_temperature")
        thr = self.hyper("stopping_threshold")
        lik_std = self.hyper("vae_likelihood_std")
        batched = self._batched_vae(B)
        # hoisted x-projection of the LSTM input (input is loop-invariant in AIR)
        with self._timed("lstm_x_projection"):
            gemm([Xl], [Wx], [ws.Gx], B, 4 * H, NX, NX, 4 * H, 4 * H)
        if side is not None:
            torch.cuda.current_stream().wait_event(pre_done)
        w1 = [self._P(h + "/hidden/weights") for h in self._HEADS]
        b1 = [self._P(h + "/hidden/biases") for h in self._HEADS]
        w2 = [self._P(h + "/output/weights") for h in self._HEADS]
        b2 = [self._P(h + "/output/biases") for h in self._HEADS]
        # batched VAE: the LSTM chain first, then every step's heads over T*B
        # rows and every step's scalars in one launch each (the heads read h_t
        # only; mog_air_step_forward_steps)
        steps_all = batched and T <= 8 and self.STEPS_ONE_LAUNCH
        for t in range(T):
            if t == 0:
                _ops.lstm_cell_forward_(ws.Gx, bK, None, ws.c[0], ws.h[0], B, H)
            else:
                gemm([ws.h[t - 1]], [Wh], [ws.G[t]], B, 4 * H, H, H, 4 * H, 4 * H, bias=[bK],
                     Cin=[ws.Gx])
                _ops.lstm_cell_forward_(ws.G[t], None, ws.c[t - 1], ws.c[t], ws.h[t], B, H)
            if steps_all:
                continue
            hid_t = [ws.hid[z, t] for z in range(5)]
            gemm([ws.h[t]] * 5, w1, hid_t, B, HS, H, H, HS, HS, epi=EPI_RELU, bias=b1)
            bias_t = float(self.marginal[t]) if self.marginal is not None else 0.0
            rec = ws.rec[t]
            _ops.air_step_forward_(
                B, HS, HS, t, self.train, self.marginal is not None, thr, temperature, prior_lo,
                bias_t, float(self.scale_prior_mean), float(self.scale_prior_variance),
                self.scale_prior_log_variance, float(self.shift_prior_mean),
                float(self.shift_prior_variance), self.shift_prior_log_variance, hid_t, w2, b2,
                ws.eps_scale[t], ws.eps_shift[t], ws.u[t], ws.stop, ws.runloss, ws.digits,
                ws.live, rec, ws.th_f[t], ws.th_b[t], ws.scale[t], ws.shift[t], ws.zprob[t],
                ws.zkl[t], ws.skl[t], ws.shkl[t], ws.zmask[t], ws.zval[t], ws.zc[t],
                self._prior_arg())
            if self.live_hook is not None:
                self.live_hook(ws.live, t)
            if batched:
                continue
            if self.fused_step:
                with self._timed("stn_vae_step"):
                    self._step_fused(X, ws, t, float(lik_std), save=need_grad)
                continue
            # STN read -> glimpse VAE (air_model.py:523-550, vae.py:5-48)
            self._vae_encoder(X, ws, t, t + 1, ws.runloss)
            self._vae_decoder(ws, float(lik_std), t, t + 1)
            # STN write + masked canvas accumulation (air_model.py:580-588, 665-675)
            ops.stn_forward(ws.r[t], ws.th_b[t], (C, C), out=ws.canvas, z=ws.zval[t],
                            mask=ws.zmask[t], accumulate=True)
        if steps_all:
            TB = T * B
            gemm([ws.h.view(TB, H)] * 5, w1, [ws.hid[z].view(TB, HS) for z in range(5)], TB, HS,
                 H, H, HS, HS, epi=EPI_RELU, bias=b1)
            biases = [float(self.marginal[t]) if self.marginal is not None else 0.0
                      for t in range(T)]
            _ops.air_step_forward_steps_(
                T, B, HS, HS, self.train, self.marginal is not None, thr, temperature, prior_lo,
                biases, float(self.scale_prior_mean), float(self.scale_prior_variance),
                self.scale_prior_log_variance, float(self.shift_prior_mean),
                float(self.shift_prior_variance), self.shift_prior_log_variance,
                [ws.hid[z] for z in range(5)], w2, b2, ws.eps_scale, ws.eps_shift, ws.u, ws.stop,
                ws.digits, ws.live, ws.rec, ws.th_f, ws.th_b, ws.scale, ws.shift, ws.zprob,
                ws.zkl, ws.skl, ws.shkl, ws.zmask, ws.zval, ws.zc, self._prior_arg())
            if self.live_hook is not None:
                for t in range(T):
                    self.live_hook(ws.live, t)
        if batched:
            self._vae_forward_all(X, ws, float(lik_std), save=need_grad)
            # the running loss in the loop's order (z_pres term, scale, shift
            # and VAE KLs per step), replayed from the step records; with the
            # one-launch steps, the loop predicate live[t] applied here first
            _ops.air_runloss_(T, B, ws.rec, R_NREC * B, ws.skl, ws.shkl, ws.vkl, ws.runloss,
                              ws.live if steps_all else None)
        self._forward_loss(X, targets, ws, need_grad, outputs)

    def _parts_layout(self, B: int) -> bool:
        """Per-step canvas parts [T, B, C*C] (+ stored row ranges) summed in
        step order by the loss kernel, instead of one running canvas: the
        fused step kernel and the all-steps STN write."""
        return self.fused_step or self._batched_vae(B)

    def _eps_x_in_kernel(self, B: int) -> bool:
        """The likelihood noise eps_x is generated where it is consumed: in the
        fused step kernel (bf16) or in the fp32 output layer's epilogue (the
        batched VAE), never materialised."""
        return self.fused_step or (self.precision == "fp32" and self._batched_vae(B))

    def _batched_vae(self, B: int) -> bool:
        """AIR's VAE output never feeds the recurrence (the LSTM input is the
        image alone, air_model.py:454-456), so the glimpse VAE of every step
        can run after the loop over all T*B rows at once: taller GEMMs and one
        fused launch instead of T.  Rows of one image stay independent, so
        every output is bit-identical to the per-step schedule; the canvas is
        still accumulated in step order.  Tiles of the fused kernel must not
        straddle two steps (B % 64)."""
        return self.batch_vae and B % 64 == 0

    def _forward_loss(self, X, targets, ws, need_grad, outputs=True):
        """reconstruction loss (air_model.py:866-900) + batch means.  With
        outputs=False (train steps) the clipped reconstruction and, in the
        fused configuration, the summed canvas are not stored; the
        ``reconstruction`` / ``canvas`` accessors materialize them on demand."""
        B, C2 = ws.B, self.C2
        parts = ws.cparts
        self._loss_inputs = (X, targets)
        ws.materialized = bool(outputs)
        gscale = self._gscale(B)
        canvas = ws.canvas if (outputs or parts is None) else None
        _ops.recon_loss_(X, canvas, parts, self.max_steps if parts is not None else 0, B * C2,
                         ws.prows, self.canvas_size, ws.runloss, ws.digits, targets, B, C2,
                         float(gscale), ws.recon if outputs else None, ws.bce, ws.mse, ws.loss_b,
                         ws.acc_b if targets is not None else None,
                         ws.dcanvas if need_grad else None)
        _ops.batch_mean_(ws.loss_b, ws.acc_b if targets is not None else None, ws.mse, None, B,
                         ws.means)
        self._outputs_ready = True

    # ---------------------------------------------------------- backward ---
    def _backward(self, X: torch.Tensor, ws: _Workspace) -> None:
        """Every loop step's glimpse-path backward (STN write, VAE, STN read,
        heads) depends only on that step's records and dL/dcanvas, so it runs
        once over all T*B rows; only the LSTM chain is sequential."""
        st = self.params
        # the gradient buffer and the LSTM chain's dG sum, zeroed in one launch
        # (the fp32 x3p x-rows gradient reads every step's dG instead of the
        # sum: mog_split3_sum_bf16)
        if self._x3p_xgrad(ws.B) and not self.cnn:
            _ops.fill32_batch_([st.grad], [0])
        else:
            _ops.fill32_batch_([st.grad, ws.dGsum], [0, 0])
        self._backward_body_grouped(X, ws)

    def _backward_body(self, X: torch.Tensor, ws: _Workspace) -> None:
        B, T, H = ws.B, self.max_steps, self.rnn_units
        W = self.windows_size
        HS = self.scale_hidden_units
        TB = T * B
        K = self._P("rnn/basic_lstm_cell/kernel")
        bK = self._P("rnn/basic_lstm_cell/bias")
        Wx, Wh = K[:self.lstm_in], K[self.lstm_in:]
        w2 = [self._P(h + "/output/weights") for h in self._HEADS]
        gscale = self._gscale(B)
        prior_lo = self.hyper("z_pres_prior_log_odds")
        temperature = self.hyper("z_pres_temperature")
        # STN write backward of all steps against the shared canvas gradient
        with self._timed("stn_write_bwd", self._stn_bwd_work(TB, write=True)):
            self._stn_write_backward_all(ws)
        self._vae_decoder_backward(ws, 0, T)
        self._vae_encoder_backward(ws, 0, T, gscale)
        # The VAE weight gradients need only the activations and the VAE input
        # gradients, final here: they run on a second stream (MFMA-bound
        # split-K GEMMs) under the latency-bound STN read backward and the
        # heads' backward.  Data parallel: the main stream joins them before
        # the glimpse-side all-reduce bucket and the LSTM chain.  One GPU: the
        # heads' weight gradients follow them on the side stream and the join
        # is before Adam, so both overlap the LSTM chain (3.49 -> 3.45 ms;
        # the VAE's alone joined before Adam, heads on the main stream, was
        # measured slower in round 2: 3.74 -> 3.81 ms).
        # (measured: forking them after the STN read backward instead, so that
        # kernel runs alone, is neutral -- 3.097 / 3.094 vs 3.098 / 3.097 ms).
        # Below SIDE_MIN_BATCH everything stays on the main stream (see
        # _vae_weight_grads_async).
        # (from SIDE_MIN_BATCH the heads' concatenated W1, the B operand of
        # the dh GEMM below, is refreshed first on that stream: off the main
        # stream, which waits for it only at that GEMM)
        w1_done, vae_done = self._vae_weight_grads_async(ws, first=self._w1cat)
        # STN read backward of all steps against the shared input canvas
        with self._timed("stn_read_bwd", self._stn_bwd_work(TB, write=False)):
            ops.stn_backward(X, ws.th_f, (W, W), ws.dg_all, want_dU=False, dtheta=ws.dth_f_all,
                             n=TB)
        if self.marginal is None:
            # every step's inputs are final here (the STN backwards ran over
            # all T*B rows above): the T steps' head backward in one launch
            _ops.air_step_backward_(
                B, HS, self.train, False, temperature, prior_lo, 0.0,
                float(self.scale_prior_mean), float(self.scale_prior_variance),
                float(self.shift_prior_mean), float(self.shift_prior_variance), float(gscale),
                None, ws.rec, ws.eps_scale, ws.eps_shift, ws.dth_f_all, ws.dth_b_all, ws.dot_all,
                [ws.hid[z] for z in range(5)], w2, ws.dout[0], T * B * 2, ws.dhid, HS,
                self._prior_arg(), T)
        for t in range(T if self.marginal is not None else 0):
            hid_t = [ws.hid[z, t] for z in range(5)]
            _ops.air_step_backward_(
                B, HS, self.train, self.marginal is not None, temperature, prior_lo,
                float(self.marginal[t]) if self.marginal is not None else 0.0,
                float(self.scale_prior_mean), float(self.scale_prior_variance),
                float(self.shift_prior_mean), float(self.shift_prior_variance), float(gscale),
                None, ws.rec[t], ws.eps_scale[t], ws.eps_shift[t], ws.dth_f_all[t], ws.dth_b_all[t],
                ws.dot_all[t], hid_t, w2, ws.dout[0, t], T * B * 2, ws.dhid[t], HS,
                self._prior_arg())
        # dh[t] = sum_z dhid_z W1_z^T for every step: one plain GEMM over
        # K = 5 HS ([dhid_0 .. dhid_4] rows against [W1_0 .. W1_4]), the same
        # k-ordered chain as the per-head sum
        if w1_done is not None:
            torch.cuda.current_stream().wait_event(w1_done)
        if B < self.SIDE_MIN_BATCH and HS % 16 == 0:
            # small batch: the same chain as five k-segments read from the
            # heads' own W1 (no concatenation launch per step)
            dhid = ws.dhid.view(TB, 5 * HS)
            ops.gemm_kseg([dhid[:, z * HS:] for z in range(5)],
                          [self._P(h + "/hidden/weights") for h in self._HEADS], ws.dh, TB, H,
                          HS, 5 * HS, HS, H, transB=True)
        else:
            gemm([ws.dhid], [self._w1cat()], [ws.dh], TB, H, 5 * HS, 5 * HS, 5 * HS, H,
                 transB=True)
        heads_side = (self.grad_reducer is None and self.HEADS_WGRAD_SIDE
                      and B >= self.SIDE_MIN_BATCH)
        if heads_side:
            # one GPU, no bucket to hand over: the heads' weight gradients
            # follow the VAE's on the side stream, under the latency-bound
            # LSTM chain; the main stream joins them before Adam
            # -- on a third stream, beside the VAE's instead of queued after
            # them (fp32 step 3.10 -> 3.05 ms)
            with torch.cuda.stream(self._fork(self._stream3())):
                self._weight_grads_heads(ws)
        else:
            # the heads' and the VAE's weight gradients are final here: their
            # all-reduce bucket runs while the LSTM chain below computes
            self._weight_grads_heads(ws)
            if vae_done is not None:
                torch.cuda.current_stream().wait_event(vae_done)
            split = self._bucket_split()
            self._reduce_bucket(split, self.params.total)
        rec_early = T > 1 and heads_side and self.REC_WGRAD_SIDE
        # (cnn=True: the encoder's input gradient reads the sum in either form)
        dGsum = None if self._x3p_xgrad(B) and not self.cnn else ws.dGsum
        # a small batch's dh GEMM in DH_PARTS K slices that the next cell
        # backward adds to the heads' dh in part order (_dh_parts)
        parts = self._dh_parts(B)
        dh_parts = ws.buffer("dh_parts", (parts, B, H)) if parts else None
        for t in reversed(range(T)):
            dc_in = ws.dc[(t + 1) % 2] if t < T - 1 else None
            G_t, b_t = (ws.Gx, bK) if t == 0 else (ws.G[t], None)
            c_prev = ws.c[t - 1] if t > 0 else None
            if parts and t < T - 1:
                _ops.lstm_cell_backward_parts_(G_t, b_t, c_prev, ws.c[t], ws.dh[t], dh_parts,
                                               parts, dc_in, ws.dG[t], ws.dc[t % 2], dGsum, B, H)
            else:
                _ops.lstm_cell_backward_(G_t, b_t, c_prev, ws.c[t], ws.dh[t], dc_in, ws.dG[t],
                                         ws.dc[t % 2], dGsum, B, H)
            if t == 1 and rec_early:
                # dG[1:] is final: the recurrent rows' gradient runs beside the
                # chain's last step instead of beside the x-rows gradient
                self._weight_grads_rec_side(ws)
            if t > 0 and parts:
                kp = 4 * H // parts
                gemm([ws.dG[t][:, j * kp:] for j in range(parts)],
                     [Wh[:, j * kp:] for j in range(parts)], [dh_parts[j] for j in range(parts)],
                     B, H, kp, 4 * H, 4 * H, H, transB=True)
            elif t > 0:
                gemm([ws.dG[t]], [Wh], [ws.dh[t - 1]], B, H, 4 * H, 4 * H, 4 * H, H,
                     transB=True, Cin=[ws.dh[t - 1]])
        self._weight_grads_lstm(ws.feat if self.cnn else X, ws, side=heads_side,
                                rec_done=rec_early)
        if self.cnn:
            # dF = (sum_t dG_t) Wx^T, then the encoder's backward (main stream)
            gemm([ws.dGsum], [Wx], [ws.dF], B, self.lstm_in, 4 * H, 4 * H, 4 * H, self.lstm_in,
                 transB=True)
            with self._timed("cnn_enc_backward"):
                ops.cnn_enc_backward(X, self._cnn_tensors(), ws.pool1, ws.pool2, ws.feat, ws.dF,
                                     ws.cnn_part, self._cnn_tensors("grad"))
        if heads_side:  # (everything on the side stream: VAE, heads, dW_rec)
            torch.cuda.current_stream().wait_stream(self._side_stream())
            torch.cuda.current_stream().wait_stream(self._stream3())

    # single GPU: heads' weight gradients on the side stream (see _backward_body)
    HEADS_WGRAD_SIDE = True
    # ... and the LSTM kernel's recurrent-rows gradient beside the x-rows one
    REC_WGRAD_SIDE = True

    # -------------------------------------------------- weight gradients ---
    # (the forms and the VAE's are WeightGradients', wgrads.py)
    def _w1cat(self):
        """[W1_0 .. W1_4] side by side ([H, 5 HS]): the B operand of the heads'
        dh GEMM, refreshed when the parameters change."""
        return self._wcache.get("w1cat", self._w1cat_build)

    def _w1cat_build(self):
        buf = torch.empty((self.rnn_units, 5 * self.scale_hidden_units), device=self.device)
        return buf, lambda: torch.cat([self._P(h + "/hidden/weights") for h in self._HEADS],
                                      dim=1, out=buf)

    def _weight_grads_heads(self, ws):
        H, HS, TB = self.rnn_units, self.scale_hidden_units, ws.B * self.max_steps
        heads = list(enumerate(self._HEADS))
        dhid = ws.dhid.view(TB, 5, HS)
        g = self._G
        cols = [2 if h.startswith("shift") else 1 for _, h in heads]
        hidden = [WgradProblem(ws.h, dhid[:, zi], g(h + "/hidden/weights"),
                               g(h + "/hidden/biases"), H, HS, H, 5 * HS) for zi, h in heads]
        # open item: an open small-batch group wins over
        # the tall-K kernel here (group_first), not for the VAE / recurrent rows
        plan = self._wgrads(hidden, TB, "heads_wgrad_x3", tall=HS < 128, group_first=True)
        if plan[0].form == TALL_X3:  # (a tall plan is one launch of every problem)
            # deterministic from the split-K batch sizes on: the five hidden
            # layers on the grouped x3 kernel (splits added in order), the 1- /
            # 2-column output layers by chunk partials added in chunk order
            # (mog_heads_output_wgrad)
            _ops.heads_output_wgrad_([ws.hid[zi] for zi, _ in heads],
                                     [ws.dout[zi] for zi, _ in heads],
                                     [g(h + "/output/weights") for _, h in heads],
                                     [g(h + "/output/biases") for _, h in heads], cols, TB, HS)
            return
        # the 1-column layers, then the 2-column ones: one batched launch each
        self._wgrads([WgradProblem(ws.hid[zi], ws.dout[zi], g(h + "/output/weights"),
                                   g(h + "/output/biases"), HS, k, HS, 2)
                      for k in (1, 2) for zi, h in heads if cols[zi] == k], TB)

    def _x3p_xgrad(self, B):
        """fp32: the LSTM kernel's x-rows gradient on the pre-split
        three-piece form (X_GRAD_X3 = 2) from X3P_MIN_B, reading every step's
        dG (mog_split3_sum_bf16: at most 8 steps) instead of their running
        sum.  The forward's split of X, the backward's dGsum and
        _weight_grads_lstm all key on this one predicate."""
        return (self.precision == "fp32" and self.X_GRAD_X3 == 2 and B >= self.X3P_MIN_B
                and self.max_steps <= 8)

    def _weight_grads_rec_side(self, ws):
        """One GPU: the LSTM kernel's recurrent-rows gradient sum_t h[t-1]^T
        dG[t] on a side stream, forked as soon as dG[1:] is final (before the
        chain's step 0), so it overlaps that step instead of the x-rows
        gradient."""
        # (on the third stream after the heads' weight gradients: 3.06 ->
        # 3.04 ms against the side stream)
        with torch.cuda.stream(self._fork(self._stream3())):
            self._dw_rec(ws)

    def _dw_rec(self, ws):
        """The LSTM kernel's recurrent rows: gK[lstm_in:] += sum_t h[t-1]^T dG[t]
        over (T-1) B rows.  From WGRAD_TN_MIN_ROWS (either precision:
        fp32-level, and faster than the fp32 chain): on the bf16 matrix cores
        with exact three-piece splits (the grouped x3 kernel of the fp32 VAE
        weight gradients, one problem, 256 x 1024 x 16,384 at B = 8192:
        deterministic), else the fp32 split-K GEMM."""
        B, T, H, C2 = ws.B, self.max_steps, self.rnn_units, self.lstm_in
        gK = self._G("rnn/basic_lstm_cell/kernel")
        self._wgrads([WgradProblem(ws.h, ws.dG[1:], gK[C2:], None, H, 4 * H, H, 4 * H)],
                     (T - 1) * B, "rec_wgrad_x3", tall=self.REC_WGRAD_X3, check_even=False)

    def _weight_grads_lstm(self, X, ws, side=False, rec_done=False):
        """LSTM kernel / bias gradients.  Data parallel: the x-part X^T dGsum
        (2500 x 1024, 10 MB) is produced in row chunks, each handed to the
        all-reduce as soon as it is final, so the collective of chunk i runs
        under the GEMM of chunk i+1; the recurrent rows and the bias go last.
        rec_done: the recurrent rows were forked already (_weight_grads_rec_side).
        X: the LSTM's input (lstm_in wide: the canvas or the encoder's features)."""
        B, T, H, C2 = ws.B, self.max_steps, self.rnn_units, self.lstm_in
        gK = self._G("rnn/basic_lstm_cell/kernel")
        gbK = self._G("rnn/basic_lstm_cell/bias")
        if rec_done:
            pass
        elif T > 1 and side and self.REC_WGRAD_SIDE:
            self._weight_grads_rec_side(ws)
        elif T > 1:
            self._dw_rec(ws)
        chunk = self.X_GRAD_CHUNK if self.grad_reducer is not None else C2
        base = self.params.offsets[self._SCOPE_PREFIX + "rnn/basic_lstm_cell/kernel"]
        x3p = self._x3p_xgrad(B)
        if x3p:
            # the pieces of sum_t dG_t, summed in the reversed loop's order
            # without the running sum (mog_split3_sum_bf16)
            _ops.split3_sum_bf16_(ws.dG, T, B * 4 * H,
                                  ws.buffer("dG3", (3, B, 4 * H), torch.bfloat16), B, 4 * H,
                                  4 * H, 4 * H, B * 4 * H)
        m_last = 0
        for m0 in range(0, C2, chunk):
            m_last = m0
            m1 = min(C2, m0 + chunk)
            # bias gradient = colsum(sum_t dG_t) = colsum(dGsum), fused into chunk 0
            self._x_rows_grad(X, ws, gK, gbK if m0 == 0 else None, m0, m1, x3p)
            if m1 < C2:
                self._reduce_bucket(base + m0 * 4 * H, base + m1 * 4 * H)
        self._reduce_bucket(base + m_last * 4 * H, self._bucket_split())
