"""GlimpseVAE — the glimpse VAE's launch sequences (air/vae.py:5-48 behind
the STN read, air_model.py:523-550), a mixin of ModelBase shared by the AIR and
AIR-ASR models.

Every sequence is written once per precision and direction over the rows of
loop steps [t0, t1): n = (t1 - t0) * B rows from the origin of ``a[t0]`` in
each of the workspace's [T, B, ...] buffers (_rows).  One loop step is the range
[t, t + 1); AIR's batched schedule and AIR-ASR's deferred decoder are [0, T).
Rows of one image are independent, so every range gives the same bits.

Forward: ``_vae_encoder`` (STN read -> recognition layers -> latent sample)
and ``_vae_decoder`` (generative layers), or one fused launch
(``_fused_bf16_launch``, the fp32 one in ``_vae_forward_all``).  Backward:
``_vae_decoder_backward`` then ``_vae_encoder_backward``; the cotangent dm
arrives through the output sigmoid from the STN write backward
(ModelBase._stn_write_backward_all).
"""
from __future__ import annotations

import torch

from . import ops
from .ops import (BF_SIGMOID_NOISE, BF_SOFTPLUS, BF_SOFTPLUS_BWD, BF_STORE, EPI_SIGMOID_NOISE,
                  EPI_SOFTPLUS, EPI_SOFTPLUS_BWD, EPI_STORE, gemm, gemm_bf16)

_ops = ops._ops  # torch.ops.mog_air (csrc/torch_ops.cpp)


def _rows(T, t0, t1):
    """View of a [T, B, ...] workspace buffer that starts at the rows of loop
    steps [t0, t1): the kernels take an operand's origin and the row count,
    so all T steps are the buffer itself (no view made) and one step is a[t]."""
    if t1 - t0 == 1:
        return lambda a: a[t0]
    if (t0, t1) == (0, T):
        return lambda a: a
    return lambda a: a[t0:t1]


def _step_rows(T, t):
    """_rows of loop step t, or (t None) of all T steps."""
    return _rows(T, 0, T) if t is None else _rows(T, t, t + 1)


class GlimpseVAE:
    _VAE = ("recognition_1", "recognition_2", "rec_mean", "rec_log_variance", "generative_1",
            "generative_2", "gen_mean")

    def _vae_dims(self):
        R1, R2 = self.vae_recognition_units
        G1, G2 = self.vae_generative_units
        return self.W2, R1, R2, self.vae_latent_dimensions, G1, G2

    def _vae_w(self):
        return {n: self._P("vae/" + n + "/weights") for n in self._VAE}

    def _vae_b(self):
        return {n: self._P("vae/" + n + "/biases") for n in self._VAE}

    # ----------------------------------------------------- weight copies ---
    # bf16 configuration: VAE GEMM operands bf16 (fp32 accumulate), activations
    # stored bf16 (post-activation only: softplus' = 1 - exp(-softplus)), the
    # LSTM / heads / STN / canvas / losses stay fp32.
    @staticmethod
    def _pad8(n):
        return (n + 7) // 8 * 8

    def _pack_bf16(self):
        """Refresh the bf16 weight packs after a parameter update (one batched
        launch): wn[name] = W [in][out8] (dX B operand) and either
        wf[name] = W^T in MFMA B-fragment order (fused step kernel) or
        wt[name] = W^T [out][in8] (unfused forward GEMMs)."""
        self._wcache.get("pack_bf16", self._pack_bf16_build)

    def _pack_bf16_build(self):
        bf = dict(device=self.device, dtype=torch.bfloat16)
        self._wt, self._wn, self._wf = {}, {}, {}
        srcs, dsts, dims = [], [], []
        for n in self._VAE:
            w = self._P("vae/" + n + "/weights")
            I, O = w.shape
            wn = self._wn[n] = torch.zeros((I, self._pad8(O)), **bf)
            if self.fused_step:
                Np, Kp = (O + 15) // 16 * 16, (I + 31) // 32 * 32
                wf = self._wf[n] = torch.zeros((Np, Kp), **bf)
                fwd, fdims = wf, [I, O, O, Np, Kp, Kp, 2]
            else:
                wt = self._wt[n] = torch.zeros((O, self._pad8(I)), **bf)
                fwd, fdims = wt, [I, O, O, O, wt.shape[1], wt.shape[1], 1]
            srcs += [w, w]
            dsts += [fwd, wn]
            dims += fdims + [I, O, O, I, wn.shape[1], wn.shape[1], 0]
        return dsts, lambda: _ops.cvt_bf16_batch_(srcs, dsts, dims)

    def _pack_f32(self):
        """Refresh the fp32 MFMA B-fragment packs of the VAE weights (the fp32
        fused step's weight operand) after a parameter update: one launch."""
        self._wcache.get("pack_f32", self._pack_f32_build)

    def _pack_f32_build(self):
        ws_, ks, ns, outs = [], [], [], []
        for n in self._VAE:
            w = self._P("vae/" + n + "/weights")
            K, N = w.shape
            ws_.append(w)
            ks.append(int(K))
            ns.append(int(N))
            outs.append(torch.empty(((K + 15) // 16) * ((N + 15) // 16) * 256,
                                    device=self.device))
        self._wf32 = outs
        return outs, lambda: _ops.pack_frag_f32_(ws_, ks, ns, outs)

    def _vae_wT(self):
        """W^T of rec_mean, rec_log_variance [Z][R2] and generative_1 [G1][Z],
        transposed in one launch when the parameters changed."""
        return self._wcache.get("vae_wT", self._vae_wT_build)

    def _vae_wT_build(self):
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        buf = [torch.empty((Z, R2), device=self.device), torch.empty((Z, R2), device=self.device),
               torch.empty((G1, Z), device=self.device)]
        return buf, lambda: _ops.transpose32_batch_(
            buf, [self._P("vae/" + n + "/weights") for n in
                  ("rec_mean", "rec_log_variance", "generative_1")])

    def _latent_nt(self, rows):
        """The fp32 latent layers as NT products of W^T copies (_vae_wT) below
        SIDE_MIN_BATCH rows of the call: their N = Z / K = Z miss the LDS-DMA
        alignment, and their row-major form ran on 64 x 64 tiles, a few
        workgroups; the same k-ordered chains, so the same bits."""
        return self.vae_latent_dimensions % 4 != 0 and rows < self.SIDE_MIN_BATCH

    # fp32 configuration: the VAE input gradients dX = dY W^T of the 256- to
    # 784-wide layers on the bf16 matrix cores with exact three-piece splits
    # (gemm_x3.hip NT form: dY split in the kernel, W split once per optimizer
    # step) -- the chain is on the step's critical path; fp32-level accuracy
    # like the weight gradients.  False: the fp32 MFMA GEMMs.
    VAE_DX_X3 = True
    _X3_DX = ("gen_mean", "generative_2", "recognition_2", "recognition_1")

    def _w3(self):
        """The three bf16 pieces of the VAE weights the x3 input gradients read
        (W [in][out] -> [3][in][out]), refreshed when the parameters change."""
        return self._wcache.get("w3", self._w3_build)

    def _w3_build(self):
        buf = {}
        for n in self._X3_DX:
            I, O = self._P("vae/" + n + "/weights").shape
            buf[n] = torch.empty((3, I, O), device=self.device, dtype=torch.bfloat16)

        def refresh():
            for n in self._X3_DX:
                w = self._P("vae/" + n + "/weights")
                I, O = w.shape
                ops.split3_bf16(w, buf[n], I, O, O, O, I * O)
        return buf, refresh

    def _dx(self, dY, name, out, M, N, K, aux=None):
        """out[M,N] = dY W^T (W = vae/name/weights [N][K]) [* sigmoid(aux)]."""
        if self.VAE_DX_X3 and K % 8 == 0 and N % 4 == 0 and M >= self.X3_DX_MIN_ROWS:
            w3 = self._w3()[name]
            # six bf16 MFMA products per fp32 product (gemm_x3.hip)
            with self._timed("vae_dgrad_x3", ("mfma", 2.0 * M * N * K, "fp32", "x3")):
                ops.gemm_x3_nt(dY, w3, N * K, out, M, N, K, K, K, N, aux=aux,
                               ldaux=N if aux is not None else 0)
            return
        with self._timed("vae_dgrad_f32", ("mfma", 2.0 * M * N * K, "fp32")):
            gemm([dY], [self._P("vae/" + name + "/weights")], [out], M, N, K, K, K, N, transB=True,
                 epi=EPI_SOFTPLUS_BWD if aux is not None else EPI_STORE,
                 aux=[aux] if aux is not None else None, ldaux=N if aux is not None else 0)

    # ----------------------------------------------------------- forward ---
    def _vae_encoder(self, X, ws, t0, t1, runloss=None):
        """STN read of the shared input canvas -> recognition layers -> latent
        sample of loop steps [t0, t1).  runloss: the running loss the sample
        kernel adds the VAE KL to (the loop's per-step order; None where
        air_runloss_ replays it afterwards or nothing reads it)."""
        B, W = ws.B, self.windows_size
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        n, v, vb = (t1 - t0) * B, _rows(self.max_steps, t0, t1), self._vae_b()
        # (stn_forward wants theta as [n, 6]; every other operand is an origin)
        if self.precision == "bf16":
            self._pack_bf16()
            wt, Zp = self._wt, self._pad8(Z)
            ops.stn_forward(X, v(ws.th_f).view(n, 6), (W, W), out=v(ws.gb), n=n)
            gemm_bf16([v(ws.gb)], [wt["recognition_1"]], [v(ws.a1b)], n, R1, W2, W2, W2, R1,
                      epi=BF_SOFTPLUS, bias=[vb["recognition_1"]])
            gemm_bf16([v(ws.a1b)], [wt["recognition_2"]], [v(ws.a2b)], n, R2, R1, R1, R1, R2,
                      epi=BF_SOFTPLUS, bias=[vb["recognition_2"]])
            gemm_bf16([v(ws.a2b), v(ws.a2b)], [wt["rec_mean"], wt["rec_log_variance"]],
                      [v(ws.mu), v(ws.lv)], n, Z, R2, R2, R2, Z, epi=BF_STORE,
                      bias=[vb["rec_mean"], vb["rec_log_variance"]])
            self._vae_sample(ws, v, n, v(ws.zb), Zp, runloss)
            return
        vw = self._vae_w()
        ops.stn_forward(X, v(ws.th_f).view(n, 6), (W, W), out=v(ws.g), n=n)
        gemm([v(ws.g)], [vw["recognition_1"]], [v(ws.a1)], n, R1, W2, W2, R1, R1,
             epi=EPI_SOFTPLUS, bias=[vb["recognition_1"]])
        gemm([v(ws.a1)], [vw["recognition_2"]], [v(ws.a2)], n, R2, R1, R1, R2, R2,
             epi=EPI_SOFTPLUS, bias=[vb["recognition_2"]])
        nt = self._latent_nt(n)
        gemm([v(ws.a2), v(ws.a2)],
             self._vae_wT()[:2] if nt else [vw["rec_mean"], vw["rec_log_variance"]],
             [v(ws.mu), v(ws.lv)], n, Z, R2, R2, R2 if nt else Z, Z, transB=nt,
             bias=[vb["rec_mean"], vb["rec_log_variance"]])
        self._vae_sample(ws, v, n, None, 0, runloss)

    def _vae_sample(self, ws, v, n, zb, ldzb, runloss):
        _ops.vae_sample_forward_(n, self.vae_latent_dimensions, float(self.vae_prior_mean),
                                 float(self.vae_prior_variance), self.vae_prior_log_variance,
                                 v(ws.mu), v(ws.lv), v(ws.eps_z), v(ws.z), zb, ldzb, v(ws.zmask),
                                 runloss, v(ws.vkl))

    def _vae_decoder(self, ws, lik_std, t0, t1):
        """Generative layers of loop steps [t0, t1): z -> r, the output
        sigmoid with the likelihood noise eps_x added in the last epilogue."""
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        n, v, vb = (t1 - t0) * ws.B, _rows(self.max_steps, t0, t1), self._vae_b()
        if self.precision == "bf16":
            wt, Zp = self._wt, self._pad8(Z)
            gemm_bf16([v(ws.zb)], [wt["generative_1"]], [v(ws.d1b)], n, G1, Zp, Zp, Zp, G1,
                      epi=BF_SOFTPLUS, bias=[vb["generative_1"]])
            gemm_bf16([v(ws.d1b)], [wt["generative_2"]], [v(ws.d2b)], n, G2, G1, G1, G1, G2,
                      epi=BF_SOFTPLUS, bias=[vb["generative_2"]])
            gemm_bf16([v(ws.d2b)], [wt["gen_mean"]], [v(ws.r)], n, W2, G2, G2, G2, W2,
                      epi=BF_SIGMOID_NOISE, bias=[vb["gen_mean"]], aux=[v(ws.eps_x)], ldaux=W2,
                      aux_scale=lik_std)
            return
        vw = self._vae_w()
        nt = self._latent_nt(n)
        gemm([v(ws.z)], [self._vae_wT()[2] if nt else vw["generative_1"]], [v(ws.d1)], n, G1, Z,
             Z, Z if nt else G1, G1, transB=nt, epi=EPI_SOFTPLUS, bias=[vb["generative_1"]])
        gemm([v(ws.d1)], [vw["generative_2"]], [v(ws.d2)], n, G2, G1, G1, G2, G2,
             epi=EPI_SOFTPLUS, bias=[vb["generative_2"]])
        if ws.eps_x_offset is not None:
            # eps_x of steps t0.. generated in the epilogue: [T, B, W2] fill order
            ops.gemm_sigmoid_philox(v(ws.d2), vw["gen_mean"], v(ws.r), vb["gen_mean"], n, W2, G2,
                                    G2, W2, W2, lik_std, self.noise_seed,
                                    ws.eps_x_offset + t0 * ws.B * W2 // 4)
        else:
            gemm([v(ws.d2)], [vw["gen_mean"]], [v(ws.r)], n, W2, G2, G2, W2, W2,
                 epi=EPI_SIGMOID_NOISE, bias=[vb["gen_mean"]], aux=[v(ws.eps_x)], ldaux=W2,
                 aux_scale=lik_std)

    FUSED_F32_MIN_ROWS = 8192

    def _vae_forward_all(self, X, ws, lik_std, t0=0, t1=None, save=True):
        """The glimpse VAE (STN read -> VAE -> STN write into the canvas
        parts) of loop steps [t0, t1) as one set of launches over their rows.
        save=False: no backward follows (the fused kernels skip the saved
        activations)."""
        B, C, W = ws.B, self.canvas_size, self.windows_size
        t1 = self.max_steps if t1 is None else t1
        TB, W2 = (t1 - t0) * B, self.W2
        r_ = lambda a: a[t0:t1]  # noqa: E731
        if self.fused_step:
            self._pack_bf16()  # (outside the timed launch)
            # forward only (no backward follows): the backward's saved
            # activations are not written (vae_step.hip moves its own bytes)
            sv = r_ if save else (lambda a: None)  # noqa: E731
            with self._timed("stn_vae_step_all"):
                self._fused_bf16_launch(X, ws, lik_std, t0, TB, r_, sv, sv(ws.gb), None, B)
            return
        # the fused fp32 kernel runs one 32-row tile per workgroup with a long
        # serial chain per tile (~200 us): below one tile per CU (T*B < 8192
        # rows, e.g. the reference's batch of 64) the unfused launches, which
        # spread every layer over the chip, finish first -- same bits either way
        if self.precision == "fp32" and self.fused_f32 and TB >= self.FUSED_F32_MIN_ROWS:
            self._pack_f32()
            gen = ws.eps_x_offset is not None
            off = ws.eps_x_offset + t0 * B * (W2 // 4) if gen else 0
            bias = [self._P("vae/" + n + "/biases") for n in self._VAE]
            # (the pre-activations are not stored: None in their slots)
            saved = [r_(getattr(ws, n)) if save and n is not None else None
                     for n in ("g", None, "a1", None, "a2", "mu", "lv", None, "d1", None, "d2")]
            with self._timed("stn_vae_step_f32_all"):
                _ops.stn_vae_step_f32_(TB, C, X, r_(ws.th_f), r_(ws.th_b), r_(ws.zmask),
                                       r_(ws.zval), r_(ws.eps_z), r_(ws.eps_x),
                                       ops._i64(self.noise_seed), ops._i64(off), gen, self._wf32,
                                       bias, lik_std, float(self.vae_prior_mean),
                                       float(self.vae_prior_variance), self.vae_prior_log_variance,
                                       r_(ws.cparts), r_(ws.prows), None, r_(ws.vkl), saved,
                                       r_(ws.z), r_(ws.r), B)
            return
        self._vae_encoder(X, ws, t0, t1)
        self._vae_decoder(ws, lik_std, t0, t1)
        # STN write of every step into its canvas part (air_model.py:580-588);
        # the loss kernel adds the parts in step order (:665-675)
        _ops.stn_write_parts_(r_(ws.r), TB, W, W, r_(ws.th_b), C, C, r_(ws.zval),
                              r_(ws.zmask), r_(ws.cparts), r_(ws.prows))

    def _fused_bf16_launch(self, X, ws, lik_std, t0, n, r_, sv, gb, runloss, x_period=0):
        """STN read + VAE + latent sample/KL + STN write into the canvas parts
        in one launch (vae_step.hip; same arithmetic as the unfused bf16
        sequence) over the n rows from loop step t0 on that the views r_ select
        (sv: the same, or None for the activations only a backward reads;
        x row = row % x_period)."""
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        self._pack_bf16()
        if self.windows_size != 28 or (R1, R2, Z, G1, G2) != (512, 256, 50, 256, 512):
            raise ValueError("the fused step kernel is compiled for the reference VAE shape")
        wt = [self._wf[k] for k in self._VAE]
        gen = ws.eps_x_offset is not None
        off = ws.eps_x_offset + t0 * ws.B * (W2 // 4) if gen else 0
        bias = [self._P("vae/" + k + "/biases") for k in self._VAE]
        _ops.stn_vae_step_(n, self.canvas_size, X, r_(ws.th_f), r_(ws.th_b), r_(ws.zmask),
                           r_(ws.zval), r_(ws.eps_z), r_(ws.eps_x), ops._i64(self.noise_seed),
                           ops._i64(off), gen, wt, bias, lik_std, float(self.vae_prior_mean),
                           float(self.vae_prior_variance), self.vae_prior_log_variance,
                           r_(ws.cparts), r_(ws.prows), runloss, r_(ws.vkl), gb, sv(ws.a1b),
                           sv(ws.a2b), sv(ws.mu), sv(ws.lv), r_(ws.z), sv(ws.zb), sv(ws.d1b),
                           sv(ws.d2b), r_(ws.r), x_period)

    def _step_fused(self, X, ws, t, lik_std, save=True):
        """The fused bf16 launch of loop step t, adding its VAE KL to the
        running loss.  save=False: forward only, the backward's activations
        (but the glimpse gb) are not written."""
        at = lambda a: a[t]  # noqa: E731
        self._fused_bf16_launch(X, ws, lik_std, t, ws.B, at, at if save else (lambda a: None),
                                ws.gb[t], ws.runloss)

    # ---------------------------------------------------------- backward ---
    def _vae_decoder_backward(self, ws, t0, t1):
        """dm -> dd2 -> dd1 -> dz_all of loop steps [t0, t1); dm =
        SigmoidGrad(r, dr) was written by the STN write backward.  (aux = the
        softplus outputs: the epilogues take sigmoid(x) as
        1 - exp(-softplus(x)).)"""
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        n, v = (t1 - t0) * ws.B, _rows(self.max_steps, t0, t1)
        if self.precision == "bf16":
            wn = self._wn
            gemm_bf16([v(ws.dmb)], [wn["gen_mean"]], [v(ws.dd2b)], n, G2, W2, W2, W2, G2,
                      epi=BF_SOFTPLUS_BWD, aux=[v(ws.d2b)], ldaux=G2)
            gemm_bf16([v(ws.dd2b)], [wn["generative_2"]], [v(ws.dd1b)], n, G1, G2, G2, G2, G1,
                      epi=BF_SOFTPLUS_BWD, aux=[v(ws.d1b)], ldaux=G1)
            gemm_bf16([v(ws.dd1b)], [wn["generative_1"]], [v(ws.dz_all)], n, Z, G1, G1, G1, Z,
                      epi=BF_STORE)
            return
        self._dx(v(ws.dm), "gen_mean", v(ws.dd2), n, G2, W2, aux=v(ws.d2))
        self._dx(v(ws.dd2), "generative_2", v(ws.dd1), n, G1, G2, aux=v(ws.d1))
        gemm([v(ws.dd1)], [self._P("vae/generative_1/weights")], [v(ws.dz_all)], n, Z, G1, G1, G1,
             Z, transB=True)

    def _vae_encoder_backward(self, ws, t0, t1, gscale):
        """dz_all (the decoder's, plus whatever the caller added: AIR-ASR's
        carry from the next step's LSTM input) -> dg_all of loop steps
        [t0, t1): the glimpse cotangent the STN read backward takes."""
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        n, v = (t1 - t0) * ws.B, _rows(self.max_steps, t0, t1)
        bf = self.precision == "bf16"
        Zp = self._pad8(Z) if bf else 0
        _ops.vae_sample_backward_(n, Z, float(self.vae_prior_mean), float(self.vae_prior_variance),
                                  float(gscale), v(ws.mu), v(ws.lv), v(ws.eps_z), v(ws.dz_all),
                                  v(ws.zmask), *((None, None, v(ws.dmub), v(ws.dlvb)) if bf else
                                                 (v(ws.dmu), v(ws.dlv), None, None)), Zp)
        if bf:
            wn = self._wn
            gemm_bf16([v(ws.dmub)], [wn["rec_mean"]], [v(ws.tmp_a2_all)], n, R2, Zp, Zp, Zp, R2,
                      epi=BF_STORE)
            gemm_bf16([v(ws.dlvb)], [wn["rec_log_variance"]], [v(ws.da2b)], n, R2, Zp, Zp, Zp, R2,
                      epi=BF_SOFTPLUS_BWD, Cin=[v(ws.tmp_a2_all)], aux=[v(ws.a2b)], ldaux=R2)
            gemm_bf16([v(ws.da2b)], [wn["recognition_2"]], [v(ws.da1b)], n, R1, R2, R2, R2, R1,
                      epi=BF_SOFTPLUS_BWD, aux=[v(ws.a1b)], ldaux=R1)
            gemm_bf16([v(ws.da1b)], [wn["recognition_1"]], [v(ws.dg_all)], n, W2, R1, R1, R1, W2,
                      epi=BF_STORE)
            return
        vw = self._vae_w()
        gemm([v(ws.dmu)], [vw["rec_mean"]], [v(ws.tmp_a2_all)], n, R2, Z, Z, Z, R2, transB=True)
        gemm([v(ws.dlv)], [vw["rec_log_variance"]], [v(ws.da2)], n, R2, Z, Z, Z, R2, transB=True,
             epi=EPI_SOFTPLUS_BWD, Cin=[v(ws.tmp_a2_all)], aux=[v(ws.a2)], ldaux=R2)
        self._dx(v(ws.da2), "recognition_2", v(ws.da1), n, R1, R2, aux=v(ws.a1))
        self._dx(v(ws.da1), "recognition_1", v(ws.dg_all), n, W2, R1)
