"""Weight gradients both models run (the TF MatMul / BiasAdd gradients of
air/vae.py:18-46 and the x rows of the LSTM kernel, air/air_model.py:454-456):
which GEMM form each runs on, how far it splits K, and on which stream
(ModelBase mixes this in; it reads the model's workspace and parameters).  The
models declare their gradients as WgradProblem lists; plan_wgrads chooses the
forms, WeightGradients._wgrads launches them.

Forms: the fp32 chain split-K GEMM (gemm_f32.hip, float atomics), the
grouped one-launch form of a small batch (gemm_group.hip), fp32 operands on
the bf16 matrix cores with exact three-piece splits (gemm_x3.hip: in-kernel
or pre-split), the grouped tall-K kernel of either operand
kind (wgrad_tn.hip) and the bf16 configuration's bf16 GEMMs (gemm_bf16.hip).
Streams: from ModelBase.SIDE_MIN_BATCH the VAE's weight gradients run on the
side stream, the heads' and the recurrent rows' on the third stream
(DESIGN.md §4.5).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import ops
from .ops import BF_ATOMIC, EPI_ATOMIC, gemm, gemm_bf16
from .vae import _step_rows

_ops = ops._ops


class WgradProblem(NamedTuple):
    """out[M,N] += X^T dY over K rows, bias += colsum(dY) (bias may be None);
    lda / ldb are the pitches of X / dY, out's is N."""
    X: torch.Tensor
    dY: torch.Tensor
    out: torch.Tensor
    bias: Optional[torch.Tensor]
    M: int
    N: int
    lda: int
    ldb: int


# the forms a launch of the plan runs on
GROUP, TALL_X3, TALL_BF16, SPLITK_F32, X3_TN, SPLITK_BF16 = (
    "group", "tall_x3", "tall_bf16", "splitk_f32", "x3_tn", "splitk_bf16")


class WgradLaunch(NamedTuple):
    form: str
    members: Tuple[int, ...]  # indices into the problem list
    splits: int               # K splits (0: the collected group has none)


def _tiles(M, N, t):
    return ((M + t - 1) // t) * ((N + t - 1) // t)


def _splitk(c, K, kstep, target, tiles):
    """K splits that bring `tiles` workgroups to about `target`, at least
    `kstep` rows each; ONE_PASS_WGRADS: one (every split-K count is from here)."""
    return 1 if c.ONE_PASS_WGRADS else max(1, min(K // kstep, (target + tiles - 1) // tiles))


def plan_wgrads(shapes, K, kind, collecting, tall, c, group_first=False, x3_tn=(),
                check_even=True):
    """The launches of one call site's weight gradients: a list of
    WgradLaunch.  No tensors, no device.

    shapes: (M, N, lda, ldb, has_bias) per problem; K: rows; kind: "fp32" or
    "bf16" operands; collecting: the small-batch group is open (fp32 only);
    tall: the call site's switch allows the x3 / tall-K forms; c: the class
    constants (WeightGradients or a model).
    group_first: an open group wins over the tall-K form (AIR's heads; the
        VAE and the recurrent rows go tall while the group collects).
    x3_tn: members that take the in-GEMM x3 form (float atomics) when the
        tall-K form is refused for an odd dimension of ANY member (the VAE's
        four 16-byte-row layers under its all-or-nothing evenness rule).
    check_even: False for the recurrent rows, which go tall unchecked (an
        odd rnn_units is then the tall kernel's invalid-argument error).
    """
    everyone = tuple(range(len(shapes)))
    if kind == "bf16":
        if tall and K >= c.WGRAD_TN_MIN_ROWS:
            return [WgradLaunch(TALL_BF16, everyone, c.WGRAD_TN_SPLITS)]
        return [WgradLaunch(SPLITK_BF16, (i,), _splitk(
            c, K, 512, c.DW_BF16_TARGET, _tiles(M, N, 128 if M >= 128 and N >= 128 else 64)))
            for i, (M, N, *_) in enumerate(shapes)]
    # the tall-K kernel reads 8-byte rows: every M and N even
    if (tall and K >= c.WGRAD_TN_MIN_ROWS and not (group_first and collecting)
            and not (check_even and any(s[0] % 2 or s[1] % 2 for s in shapes))):
        return [WgradLaunch(TALL_X3, everyone, c.WGRAD_TN_X3_SPLITS)]
    x3_ok = bool(x3_tn) and tall and K >= c.X3_MIN_ROWS
    rest = GROUP if collecting else SPLITK_F32
    runs = []  # (form, members)
    for i, s in enumerate(shapes):
        if x3_ok and i in x3_tn and s[0] % 4 == 0 and s[1] % 4 == 0:
            runs.append((X3_TN, [i]))
        # consecutive problems of one shape (both with or both without a
        # bias) share a collected group / one batched split-K launch
        elif runs and runs[-1][0] == rest and (collecting or shapes[runs[-1][1][-1]] == s):
            runs[-1][1].append(i)
        else:
            runs.append((rest, [i]))

    def splits(form, members):
        M, N = shapes[members[0]][:2]
        if form == X3_TN:
            return _splitk(c, K, 256, 512, _tiles(M, N, 128))
        return _splitk(c, K, 256, c.DW_F32_TARGET, _tiles(M, N, 64) * len(members))
    return [WgradLaunch(form, tuple(m), 0 if form == GROUP else splits(form, m))
            for form, m in runs]


class WeightGradients:
    # every weight gradient in one k pass (split-K 1, one atomic add per
    # element onto the zeroed gradient): a bitwise-reproducible step, for the
    # stream-ordering tests (tests/test_gpu_streams.py).  (The tall-K forms
    # keep their splits: they add them in order.)
    ONE_PASS_WGRADS = False

    # workgroups the split-K weight gradients aim for (bf16 sweep of 128-2048:
    # 256 best; fp32 512 / 1024 / 2048: 2048 best)
    DW_BF16_TARGET = 256
    DW_F32_TARGET = 2048

    # the grouped tall-K kernel (wgrad_tn.hip: all seven layers in one launch,
    # K split over the XCDs, partials added in order) from this many rows;
    # below it the per-layer split-K GEMMs
    WGRAD_TN_MIN_ROWS = 2048
    WGRAD_TN_SPLITS = 8
    # the x3 form: 16 splits (350 vs 427 us at 8 for the four layers at
    # 24,576 rows, scripts/wgrad_shapes.py)
    WGRAD_TN_X3_SPLITS = 16

    # fp32 configuration: the VAE weight gradients on the bf16 matrix cores
    # with exact three-piece splits (fp32-level accuracy, as the LSTM x-rows
    # gradient): all seven layers on the grouped tall-K
    # kernel, or, when a dimension is odd, those whose operands are 16-byte
    # rows (M, N multiples of 4: the 784/512/256-wide layers, 98 % of the
    # flops) split inside the GEMM (gemm_x3.hip); False keeps them on the
    # fp32 split-K GEMM
    VAE_WGRAD_X3 = True

    # the in-GEMM x3 form from this many rows: below it (the reference's batch
    # of 64: 192 rows) its 128 x 128 tiles leave most CUs idle, and the fp32
    # GEMMs' small-M tiles finish first
    X3_MIN_ROWS = 2048
    # the NT input-gradient form from this many rows (the AIR step's T*B =
    # 24,576 and the ASR step's per-step 8,192): below it its 128 x 128 tiles
    # leave CUs idle and the fp32 GEMM finishes first.  (Round 4, after the
    # NT load fixes: ASR fp32 step 9.46 -> 9.43 ms with 8,192 in; before
    # them the NT form lost there, 9.6 -> 10.1 ms.)
    X3_DX_MIN_ROWS = 8192

    def _wgrads(self, problems, K, tag=None, tall=False, kind="fp32", **rules):
        """Run `problems` (WgradProblem list) over K rows on the forms
        plan_wgrads chooses; returns the plan.  tag: the _timed tag of the
        call site's x3 / tall-K launches; rules: plan_wgrads' named
        irregularities."""
        plan = plan_wgrads([(p.M, p.N, p.lda, p.ldb, p.bias is not None) for p in problems], K,
                           kind, self._wgroup is not None, tall, self, **rules)
        for form, members, splits in plan:
            ps = [problems[i] for i in members]
            p = ps[0]
            X, dY, out = [q.X for q in ps], [q.dY for q in ps], [q.out for q in ps]
            bias = [q.bias for q in ps]
            flops = sum(2.0 * K * q.M * q.N for q in ps)
            if form == GROUP:  # collected: one grouped launch ends the backward
                for q in ps:
                    self._wgroup.add(q.X, q.dY, q.out, q.M, q.N, K, q.lda, q.ldb, q.N, q.bias)
            elif form in (TALL_X3, TALL_BF16):
                x3 = form == TALL_X3
                work = ("mfma", flops, "fp32", "x3") if x3 else ("mfma", flops, "bf16")
                with self._timed(tag, work):
                    (ops.wgrad_tn_x3 if x3 else ops.wgrad_tn_bf16)(
                        X, dY, out, bias, [(q.M, q.N, q.lda, q.ldb, q.N) for q in ps], K, splits)
            elif form == SPLITK_F32:
                with self._timed("wgrad_f32", ("mfma", flops, "fp32")):
                    gemm(X, dY, out, p.M, p.N, K, p.lda, p.ldb, p.N, transA=True, epi=EPI_ATOMIC,
                         splitk=splits, colsum=None if p.bias is None else bias)
            elif form == X3_TN:
                # six bf16 MFMA products per fp32 product (gemm_x3.hip); float
                # atomics for the 19-64 split-K partials of these <= 0.4
                # M-element outputs (through the workspace: 160 -> 229 us per
                # launch in the step)
                with self._timed(tag, ("mfma", flops, "fp32", "x3")):
                    ops.gemm_x3_tn(p.X, p.dY, p.out, p.M, p.N, K, p.lda, p.ldb, p.N,
                                   splitk=splits, colsum=p.bias, reduce=False)
            else:
                with self._timed("wgrad_bf16", ("mfma", flops, "bf16")):
                    gemm_bf16(X, dY, out, p.M, p.N, K, p.lda, p.ldb, p.N, tn=True,
                              epi=BF_ATOMIC, splitk=splits, colsum=bias)
        return plan

    def _vae_weight_grads(self, ws, t=None):
        """The VAE weight gradients of the model's precision over all T*B
        rows, or over loop step t's B rows (accumulated: the per-step form of
        AIR-ASR).  From WGRAD_TN_MIN_ROWS the seven layers run in ONE grouped
        launch (wgrad_tn.hip: K split over the XCDs, partials added in order
        -- deterministic; fp32: the x3 form, fp32-level accuracy)."""
        K = ws.B * self.max_steps if t is None else ws.B
        v = _step_rows(self.max_steps, t)
        W2, R1, R2, Z, G1, G2 = self._vae_dims()
        # the bf16 operands are the fp32 buffers' names + "b", their latent
        # pitch padded to 8
        bf = self.precision == "bf16"
        sfx, Zp = ("b", self._pad8(Z)) if bf else ("", Z)
        # (X, dY, layer, M, N, lda, ldb) of the seven layers
        table = (("g", "da1", "recognition_1", W2, R1, W2, R1),
                 ("a1", "da2", "recognition_2", R1, R2, R1, R2),
                 ("a2", "dmu", "rec_mean", R2, Z, R2, Zp),
                 ("a2", "dlv", "rec_log_variance", R2, Z, R2, Zp),
                 ("z", "dd1", "generative_1", Z, G1, Zp, G1),
                 ("d1", "dd2", "generative_2", G1, G2, G1, G2),
                 ("d2", "dm", "gen_mean", G2, W2, G2, W2))
        probs = [WgradProblem(v(getattr(ws, x + sfx)), v(getattr(ws, dy + sfx)),
                              self._G("vae/" + name + "/weights"),
                              self._G("vae/" + name + "/biases"), M, N, lda, ldb)
                 for x, dy, name, M, N, lda, ldb in table]
        # open item: one odd dimension sends the four wide
        # layers (x3_tn) to float atomics
        self._wgrads(probs, K, "vae_wgrad_bf16" if bf else "vae_wgrad_x3",
                     tall=bf or self.VAE_WGRAD_X3, kind=self.precision, x3_tn=(0, 1, 5, 6))

    def _vae_weight_grads_async(self, ws, first):
        """The VAE weight gradients on the side stream (ordered after
        everything issued so far on the current stream), behind ``first()``
        (a launch the main stream needs sooner: AIR's refresh of the heads'
        W1); returns the events that mark ``first`` and their completion.
        Below SIDE_MIN_BATCH they run in line on the current stream, without
        ``first`` (events None): at the reference's batch of 64 the launches
        are a few microseconds each, too short to hide a cross-stream wait."""
        if ws.B < self.SIDE_MIN_BATCH:
            self._vae_weight_grads(ws)
            return None, None
        side = self._fork(self._side_stream())
        with torch.cuda.stream(side):
            first()
            first_done = torch.cuda.Event()
            first_done.record(side)
            self._vae_weight_grads(ws)
            done = torch.cuda.Event()
            done.record(side)
        return first_done, done

    # fp32 configuration: the x-part of the LSTM kernel gradient on the bf16
    # matrix cores with exact three-piece operand splits (gemm_x3.hip,
    # DESIGN.md §4.4).  2 (default): the operands split once per step, X on
    # the side stream under the x-projection, dG before the GEMM (gemm_x3p_tn:
    # 244 vs 428 us stand-alone, step 3.44 -> 3.37 ms); 1: split inside the
    # GEMM (318 us, no change in the step); 0: the fp32 MFMA split-K GEMM.
    X_GRAD_X3 = 2
    # the pre-split form from this batch in the AIR model (_x3p_xgrad; the
    # AIR-ASR model's gate is _x3_asr): below it (the reference's batch of 64)
    # the two split launches cost more than the fp32 chain's K = B pass
    # (batch 64: x3p 12.3 + splits 9.6 us)
    X3P_MIN_B = 256
    X3_SPLITK = 8

    # rows of the x-part of the AIR LSTM kernel gradient per all-reduce bucket
    # (multiple of the 64-row GEMM tile; data parallel only)
    X_GRAD_CHUNK = 640

    # the LSTM kernels' recurrent-rows gradients (AIRModel._dw_rec, the AIR-ASR
    # model's _u_rows_wgrad) may take the grouped x3 kernel (plan_wgrads' tall)
    REC_WGRAD_X3 = True

    def _x_split3(self, X, ws):
        """X (the LSTM's loop-invariant input, lstm_in wide) in three exact
        bf16 pieces [3][B][C2p] (ws.X3): the A operand of the pre-split x-rows
        gradient, split once per step in the forward's prologue (X is the
        step's input, final before the x-projection)."""
        B, C2 = ws.B, self.lstm_in
        C2p = self._pad8(C2)
        ops.split3_bf16(X, ws.buffer("X3", (3, B, C2p), torch.bfloat16), B, C2, C2, C2p, B * C2p)

    def _x_rows_grad(self, X, ws, gK, bias_out, m0, m1, x3p):
        """Rows [m0, m1) of the LSTM kernel's x-rows gradient gK[:C2] += X^T
        sum_t dG_t (the x input is loop-invariant), bias_out += its column
        sums.  bf16: bf16 operands (fp32 accumulate; the forward x-projection
        stays fp32).  fp32: on the bf16 matrix cores from exact three-piece
        splits of both operands (gemm_x3.hip, DESIGN.md §4.4: fp32-level
        accuracy) -- x3p: the pieces the model prepared in ws.X3 / ws.dG3;
        X_GRAD_X3 = 1: split inside the GEMM -- or the fp32 split-K chain.
        (The GEMM of every chunk is tagged; the operand conversions / splits
        are other launches.)  X is lstm_in wide."""
        B, H, C2 = ws.B, self.rnn_units, self.lstm_in
        if self.precision == "bf16":
            return self._x_grad_bf16(X, ws, gK, bias_out, m0, m1)
        if not x3p and self.X_GRAD_X3 != 1:
            return self._wgrads([WgradProblem(X[:, m0:], ws.dGsum, gK[m0:m1], bias_out, m1 - m0,
                                              4 * H, C2, 4 * H)], B)
        splitk = _splitk(self, B, 256, self.X3_SPLITK, 1)
        with self._timed("lstm_x_projection_grad",
                         ("mfma", 2.0 * B * (m1 - m0) * 4 * H, "fp32", "x3")):
            if x3p:
                C2p = self._pad8(C2)
                ops.gemm_x3p_tn(ws.X3.view(-1)[m0:], B * C2p, ws.dG3, B * 4 * H, gK[m0:m1],
                                m1 - m0, 4 * H, B, C2p, 4 * H, 4 * H, splitk=splitk,
                                colsum=bias_out, reduce=True)
            else:
                ops.gemm_x3_tn(X[:, m0:], ws.dGsum, gK[m0:m1], m1 - m0, 4 * H, B, C2, 4 * H,
                               4 * H, splitk=splitk, colsum=bias_out)

    def _x_bf16(self, X, ws):
        """X in bf16 [B][C2p] (zero pad columns): the A operand of the bf16
        configuration's x-rows gradient, converted once per step -- in the
        forward's side-stream prologue from SIDE_MIN_BATCH (X is the step's
        input, final before the x-projection)."""
        B, C2 = ws.B, self.C2
        C2p = self._pad8(C2)
        Xb = ws.buffer("Xb", (B, C2p), torch.bfloat16)
        _ops.cvt_bf16_batch_([X], [Xb], [B, C2, C2, B, C2p, C2p, 0])
        ws.xb_fresh = True

    def _x_grad_bf16(self, X, ws, gK, bias_out, m0, m1):
        """The bf16 configuration's x-rows gradient X^T dGsum on gemm_x3p_tn's
        one-piece form (plain bf16 operands, 128 x 128 tiles): X was
        converted in the forward (_x_bf16), dGsum is converted here."""
        B, H, C2 = ws.B, self.rnn_units, self.C2
        C2p = self._pad8(C2)
        if m0 == 0:
            if not ws.xb_fresh:  # (no conversion in this step's forward)
                self._x_bf16(X, ws)
            ws.xb_fresh = False
            if ws.xb_ready is not None:  # (converted on the side stream)
                torch.cuda.current_stream().wait_event(ws.xb_ready)
                ws.xb_ready = None
            dGsumb = ws.buffer("dGsumb", (B, 4 * H), torch.bfloat16)
            _ops.cvt_bf16_batch_([ws.dGsum], [dGsumb], [B, 4 * H, 4 * H, B, 4 * H, 4 * H, 0])
        # split-K 8 at B = 8192, partials summed through the workspace
        # (scripts/x1_sweep.py, us for 1/2/3/4/6/8 splits: 138/84/77/73/73/72;
        # with float atomics 77/76/81/88 from 3 splits)
        with self._timed("lstm_x_projection_grad", ("mfma", 2.0 * B * (m1 - m0) * 4 * H, "bf16")):
            ops.gemm_x3p_tn(ws.Xb.view(-1)[m0:], 0, ws.dGsumb, 0, gK[m0:m1], m1 - m0, 4 * H, B,
                            C2p, 4 * H, 4 * H, splitk=_splitk(self, B, 1024, 8, 1),
                            colsum=bias_out, npieces=1)
