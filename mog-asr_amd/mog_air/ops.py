"""Typed wrappers of the HIP entry points over torch device tensors.

Every launch goes through the PyTorch-ROCm custom operators torch.ops.mog_air.*
(csrc/torch_ops.cpp, a TORCH_LIBRARY fragment over the C ABI of libmog_air.so)
on torch's current HIP stream.  Arguments are validated here (device, dtype,
contiguity, shape) before any launch, so a shape error never reaches a
kernel."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib

_lib.load_torch_ops()
_ops = torch.ops.mog_air

EPI_STORE, EPI_RELU, EPI_SOFTPLUS, EPI_SIGMOID_NOISE = 0, 1, 2, 3
EPI_SOFTPLUS_BWD, EPI_ATOMIC, EPI_RELU_BWD = 4, 5, 6


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def dp(t: Optional[torch.Tensor]):
    if t is None:
        return None
    return t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a HIP device tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _opt_list(xs):
    return [] if xs is None else list(xs)


def gemm(A: Sequence[torch.Tensor], B: Sequence[torch.Tensor], C: Sequence[torch.Tensor],
         M: int, N: int, K: int, lda: int, ldb: int, ldc: int, transA=False, transB=False,
         epi=EPI_STORE, bias=None, Cin=None, Cpre=None, aux=None, ldaux=0,
         aux_scale=0.0, splitk=1, colsum=None) -> None:
    """Batched fp32 MFMA GEMM (see mog_gemm_f32).  A/B/C are sequences of
    tensors (or views) whose data_ptr is the matrix origin."""
    nb = len(C)
    assert len(A) == nb and len(B) == nb and 1 <= nb <= 8
    _ops.gemm_f32_(list(A), list(B), list(C), _opt_list(bias), _opt_list(Cin), _opt_list(Cpre),
                   _opt_list(aux), _opt_list(colsum), M, N, K, lda, ldb, ldc, ldaux,
                   bool(transA), bool(transB), epi, float(aux_scale), int(splitk))


def gemm_x3_tn(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int,
               lda: int, ldb: int, ldc: int, splitk: int = 8, colsum=None,
               reduce: bool = True) -> None:
    """C[M,N] += A^T B over K rows on the bf16 matrix cores with exact
    three-piece operand splits (fp32-level accuracy; mog_gemm_f32_x3_tn);
    colsum += column sums of B.  reduce: split-K partials summed through a
    workspace in a fixed order (deterministic); False: float atomics."""
    _ops.gemm_f32_x3_tn_(A, B, C, colsum, M, N, K, lda, ldb, ldc, int(splitk), int(reduce))


def split3_bf16(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, ld_src: int,
                ld_dst: int, piece_stride: int) -> None:
    """The three exact truncated bf16 pieces of an fp32 matrix
    (mog_split3_bf16)."""
    _ops.split3_bf16_(src, dst, rows, cols, ld_src, ld_dst, int(piece_stride))


def gemm_x3p_tn(A3: torch.Tensor, sa: int, B3: torch.Tensor, sb: int, C: torch.Tensor, M: int,
                N: int, K: int, lda: int, ldb: int, ldc: int, splitk: int = 8,
                colsum=None, npieces: int = 3, reduce: bool = True) -> None:
    """gemm_x3_tn from operands split beforehand by split3_bf16
    (mog_gemm_x3p_tn); npieces=1: plain bf16 operands, one product."""
    _ops.gemm_x3p_tn_(A3, int(sa), B3, int(sb), C, colsum, M, N, K, lda, ldb, ldc, int(splitk),
                      int(npieces), int(reduce))


def gemm_x3_nt(A: torch.Tensor, B3: torch.Tensor, sb: int, C: torch.Tensor, M: int, N: int,
               K: int, lda: int, ldb: int, ldc: int, aux=None, ldaux: int = 0) -> None:
    """C[M,N] = A B^T at fp32-level accuracy (A split into three bf16 pieces
    in the kernel, B given as split3_bf16's pieces of W [N][K]); with aux:
    C = (A B^T) * sigmoid(aux) (the softplus backward) -- mog_gemm_x3_nt."""
    _ops.gemm_x3_nt_(A, B3, int(sb), C, aux, M, N, K, lda, ldb, ldc, int(ldaux),
                     1 if aux is not None else 0)


def wgrad_tn_bf16(X: Sequence[torch.Tensor], dY: Sequence[torch.Tensor],
                  out: Sequence[torch.Tensor], colsum: Sequence[Optional[torch.Tensor]],
                  dims: Sequence[Sequence[int]], K: int, nsplit: int = 8) -> None:
    """out[i] += X[i]^T dY[i] over K rows on bf16 operands, colsum[i] += the
    column sums of dY[i], every problem in one launch (dims[i] = (M, N, lda,
    ldb, ldc)); K split nsplit ways, the splits added in order by a second
    launch: deterministic (mog_wgrad_tn_bf16)."""
    _ops.wgrad_tn_bf16_(list(X), list(dY), list(out), list(colsum),
                        [int(d) for ds in dims for d in ds], int(K), int(nsplit))


def wgrad_tn_x3(X: Sequence[torch.Tensor], dY: Sequence[torch.Tensor],
                out: Sequence[torch.Tensor], colsum: Sequence[Optional[torch.Tensor]],
                dims: Sequence[Sequence[int]], K: int, nsplit: int = 8) -> None:
    """wgrad_tn_bf16 on fp32 operands at fp32-level accuracy (exact
    three-piece bf16 splits in the kernel; mog_wgrad_tn_x3)."""
    _ops.wgrad_tn_x3_(list(X), list(dY), list(out), list(colsum),
                      [int(d) for ds in dims for d in ds], int(K), int(nsplit))


class WgradGroup:
    """Weight gradients collected over a backward pass and run as ONE grouped
    launch (mog_gemm_f32_wgrad_group): each problem is out[M,N] += X^T dY
    over K rows (+ bias_out += column sums of dY); the problems travel in the
    kernel argument (graph-capturable).  Problems that share output elements
    go to successive launches (one writer per element within a launch)."""

    def __init__(self):
        self.probs = []

    @staticmethod
    def _check(t, extent, what):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise RuntimeError(f"WgradGroup: {what} must be a float32 device tensor")
        avail = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if extent > avail:
            raise RuntimeError(f"WgradGroup: {what} holds {avail} elements, needs {extent}")

    def add(self, X, dY, out, M, N, K, lda, ldb, ldc, bias_out=None):
        if min(M, N) <= 0:
            return
        span = lambda r, c, ld: 0 if r <= 0 else (r - 1) * ld + c  # noqa: E731
        self._check(X, span(K, M, lda), "X")
        self._check(dY, span(K, N, ldb), "dY")
        self._check(out, span(M, N, ldc), "out")
        if bias_out is not None:
            self._check(bias_out, N, "bias_out")
        self.probs.append((X, dY, out, bias_out, M, N, K, lda, ldb, ldc))

    def launch(self):
        """In collection order; a problem whose output or bias range overlaps
        one already in the current launch starts the next launch (same
        stream, so the two accumulate in order)."""
        batch, ranges = [], []

        def flush():
            if batch:
                X, dY, out, bias, dims = zip(*batch)
                _ops.gemm_f32_wgrad_group_(list(X), list(dY), list(out), list(bias),
                                           [d for ds in dims for d in ds])
            batch.clear()
            ranges.clear()

        for X, dY, out, b, M, N, K, lda, ldb, ldc in self.probs:
            mine = [(out.data_ptr(), out.data_ptr() + 4 * ((M - 1) * ldc + N))]
            if b is not None:
                mine.append((b.data_ptr(), b.data_ptr() + 4 * N))
            if any(lo < h and l2 < hi for lo, hi in mine for l2, h in ranges):
                flush()
            ranges.extend(mine)
            batch.append((X, dY, out, b, (M, N, K, lda, ldb, ldc)))
        flush()
        self.probs = []


def gemm_sigmoid_philox(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, bias, M: int, N: int,
                        K: int, lda: int, ldb: int, ldc: int, scale: float, seed: int,
                        offset: int) -> None:
    """C = sigmoid((A B + bias) + scale * eps), eps generated in the epilogue
    exactly as rng_fill(seed, offset) of an [M, N] buffer would hold it
    (mog_gemm_f32_sigmoid_philox)."""
    _ops.gemm_f32_sigmoid_philox_(A, B, C, bias, M, N, K, lda, ldb, ldc, float(scale),
                                  _i64(seed), _i64(offset))


def gemm_kseg(A: Sequence[torch.Tensor], B: Sequence[torch.Tensor], C: torch.Tensor, M: int,
              N: int, kseg: int, lda: int, ldb: int, ldc: int, transB=False, Cin=None,
              epi=EPI_STORE) -> None:
    """C = sum_s A_s op(B_s) as ONE k-ordered chain (mog_gemm_f32_kseg)."""
    _ops.gemm_f32_kseg_(list(A), list(B), C, None, Cin, M, N, kseg, lda, ldb, ldc, False,
                        bool(transB), epi)


def gemm_kseg_group(probs, M: int, N: int, kseg: int, lda: int, ldb: int, ldc: int,
                    transB=False) -> None:
    """Independent k-segment chains of one shape in ONE launch
    (mog_gemm_f32_kseg_group): ``probs`` = [(A_list, B_list, C, Cin), ...],
    C_z = Cin_z + sum_s A_s op(B_s) -- the same bits as one gemm_kseg each."""
    A = [a for p in probs for a in p[0]]
    B = [b for p in probs for b in p[1]]
    _ops.gemm_f32_kseg_group_(A, B, [p[2] for p in probs], [p[3] for p in probs],
                              [len(p[0]) for p in probs], M, N, kseg, lda, ldb, ldc,
                              bool(transB))


def dense(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], out: torch.Tensor,
          epi=EPI_STORE, pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(x @ w + b), one k-ordered fp32 chain per output."""
    M, K = x.shape
    K2, N = w.shape
    assert K == K2 and out.shape == (M, N)
    gemm([x], [w], [out], M, N, K, K, N, N, epi=epi, bias=None if b is None else [b],
         Cpre=None if pre is None else [pre])
    return out


def stn_forward(U: torch.Tensor, theta: torch.Tensor, out_hw, out: Optional[torch.Tensor] = None,
                z: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                accumulate: bool = False, n: Optional[int] = None) -> torch.Tensor:
    """transformer() of air/transformer.py:18 for U [N,Hin,Win] (or [N,Hin*Win] with
    Hin=Win) and theta [N,6].  A bf16 ``out`` receives the bf16 image.  n > N:
    n images, image i reading U[i % N] (every loop step's read of one canvas)."""
    _chk(U, "U")
    _chk(theta, "theta")
    period = U.shape[0] if n is not None and n != U.shape[0] else 0
    N = U.shape[0] if n is None else n
    if U.dim() == 3:
        Hin, Win = U.shape[1], U.shape[2]
    else:
        Hin = Win = int(round(U.shape[1] ** 0.5))
        assert Hin * Win == U.shape[1]
    Ho, Wo = out_hw
    assert theta.shape == (N, 6)
    if out is None:
        out = torch.empty((N, Ho * Wo), device=U.device, dtype=torch.float32)
    assert out.numel() == N * Ho * Wo and out.is_contiguous()
    if accumulate:
        assert z is not None and mask is not None and z.shape == (N,) and mask.shape == (N,)
        assert out.dtype == torch.float32
        mode = 1
    else:
        mode = 2 if out.dtype == torch.bfloat16 else 0
    _ops.stn_forward_(U, N, Hin, Win, theta, Ho, Wo, out, z, mask, mode, period)
    return out


BF_STORE, BF_SOFTPLUS, BF_SIGMOID_NOISE, BF_SOFTPLUS_BWD, BF_ATOMIC = 0, 1, 2, 3, 4


def gemm_bf16(A, B, C, M: int, N: int, K: int, lda: int, ldb: int, ldc: int, tn=False,
              epi=BF_STORE, bias=None, Cin=None, aux=None, ldaux=0, aux_scale=0.0, splitk=1,
              colsum=None) -> None:
    """Batched bf16-operand MFMA GEMM (see mog_gemm_bf16); output dtype is C's."""
    nb = len(C)
    assert len(A) == nb and len(B) == nb and 1 <= nb <= 8
    _ops.gemm_bf16_(list(A), list(B), list(C), _opt_list(bias), _opt_list(Cin), _opt_list(aux),
                    _opt_list(colsum), M, N, K, lda, ldb, ldc, ldaux, bool(tn), epi,
                    float(aux_scale), int(splitk))


def stn_backward(U: torch.Tensor, theta: torch.Tensor, out_hw, G: torch.Tensor,
                 gscale: Optional[torch.Tensor] = None, want_dU=True, want_dtheta=True,
                 want_dot=False, dU=None, dtheta=None, dot=None, n: Optional[int] = None,
                 dm: Optional[torch.Tensor] = None):
    """Gradient of transformer().  ``n`` images (default U's); when U or G
    holds fewer rows than ``n``, image i reads row i % rows (several loop
    steps of one batch against the shared canvas or canvas gradient).

    ``dm`` (bf16 or fp32 [N, Hin*Win], U = the VAE output sigmoid r): the
    input gradient is taken on through the sigmoid (vae.py:44-46) and stored
    there instead of dU -- bit-identical to dU followed by
    mog_sigmoid_backward."""
    _chk(U, "U")
    _chk(G, "G")
    if U.dim() == 3:
        Hin, Win = U.shape[1], U.shape[2]
    else:
        Hin = Win = int(round(U.shape[1] ** 0.5))
    Ho, Wo = out_hw
    NU, NG = U.numel() // (Hin * Win), G.numel() // (Ho * Wo)
    N = NU if n is None else int(n)
    assert N % NU == 0 and N % NG == 0 and theta.numel() == 6 * N
    dev = U.device
    if dm is not None:
        assert want_dU and dU is None and NU == N
        assert dm.numel() >= N * Hin * Win
        _chk(dm, "dm", dm.dtype if dm.dtype in (torch.bfloat16, torch.float32) else None)
        if want_dtheta and dtheta is None:
            dtheta = torch.empty((N, 6), device=dev, dtype=torch.float32)
        if want_dot and dot is None:
            dot = torch.empty((N,), device=dev, dtype=torch.float32)
        _ops.stn_backward_sigmoid_(U, N, Hin, Win, theta, Ho, Wo, G, gscale, dm,
                                   dtheta if want_dtheta else None, dot if want_dot else None,
                                   NG if NG < N else 0)
        return dm, dtheta, dot
    if want_dU and dU is None:
        dU = torch.empty((N, Hin * Win), device=dev, dtype=torch.float32)
    if want_dtheta and dtheta is None:
        dtheta = torch.empty((N, 6), device=dev, dtype=torch.float32)
    if want_dot and dot is None:
        dot = torch.empty((N,), device=dev, dtype=torch.float32)
    _ops.stn_backward_(U, N, Hin, Win, theta, Ho, Wo, G, gscale, dU if want_dU else None,
                       dtheta if want_dtheta else None, dot if want_dot else None,
                       NU if NU < N else 0, NG if NG < N else 0)
    return dU, dtheta, dot


CNN_CANVAS, CNN_POOL1, CNN_POOL2 = 50, 25, 12  # sides the encoder is compiled for


def cnn_images_per_wg(B: int) -> int:
    """Images one workgroup of the encoder backward sums at a batch of B by
    default: B / 512 clamped to 1..8 (mog_cnn_enc_images_per_wg)."""
    return int(_lib.load().mog_cnn_enc_images_per_wg(int(B)))


def cnn_partial_elems(B: int, images_per_wg: Optional[int] = None) -> int:
    """Floats of the encoder backward's per-workgroup partial sums for a
    batch of B (mog_cnn_enc_partial_elems)."""
    ipw = cnn_images_per_wg(B) if images_per_wg is None else int(images_per_wg)
    return int(_lib.load().mog_cnn_enc_partial_elems(int(B), ipw))


def _cnn_check(x, weights, B, F):
    _chk(x, "x")
    if x.shape != (B, CNN_CANVAS ** 2):
        raise ValueError(f"x must be [{B}, {CNN_CANVAS ** 2}], got {tuple(x.shape)}")
    shapes = ((5, 5, 1, F), (F,), (5, 5, F, F), (F,), (5, 5, F, F), (F,))
    for t, s, n in zip(weights, shapes, ("w1", "b1", "w2", "b2", "w3", "b3")):
        _chk(t, n)
        if tuple(t.shape) != s:
            raise ValueError(f"{n} must be {s}, got {tuple(t.shape)}")


def cnn_enc_forward(x: torch.Tensor, weights: Sequence[torch.Tensor], pool1: torch.Tensor,
                    pool2: torch.Tensor, feat: torch.Tensor) -> None:
    """The cnn=True encoder (mog_cnn_enc_forward): x [B, 2500], weights =
    (w1, b1, w2, b2, w3, b3) in HWIO -> feat [B, 144 F], with pool1
    [B, 625 F] and pool2 [B, 144 F] kept for the backward."""
    B, F = x.shape[0], weights[1].shape[0]
    _cnn_check(x, weights, B, F)
    for t, n, w in ((pool1, "pool1", CNN_POOL1 ** 2 * F), (pool2, "pool2", CNN_POOL2 ** 2 * F),
                    (feat, "feat", CNN_POOL2 ** 2 * F)):
        _chk(t, n)
        if t.numel() != B * w:
            raise ValueError(f"{n} must hold {B} x {w} elements, got {t.numel()}")
    _ops.cnn_enc_forward_(x, *weights, B, F, pool1, pool2, feat)


def cnn_enc_backward(x: torch.Tensor, weights: Sequence[torch.Tensor], pool1: torch.Tensor,
                     pool2: torch.Tensor, feat: torch.Tensor, dF: torch.Tensor,
                     part: torch.Tensor, grads: Sequence[torch.Tensor],
                     images_per_wg: Optional[int] = None) -> None:
    """The encoder's six gradients stored into grads = (gw1, gb1, gw2, gb2,
    gw3, gb3) from dF [B, 144 F] (mog_cnn_enc_backward); images_per_wg
    (1..8; default cnn_images_per_wg(B)): images a workgroup sums before it
    stores its partial sums; part: scratch of cnn_partial_elems(B,
    images_per_wg) floats.  Deterministic for one B and images_per_wg."""
    B, F = x.shape[0], weights[1].shape[0]
    ipw = cnn_images_per_wg(B) if images_per_wg is None else int(images_per_wg)
    if not 1 <= ipw <= cnn_images_per_wg(1 << 30):
        raise ValueError(f"images_per_wg must be 1..{cnn_images_per_wg(1 << 30)}, got {ipw}")
    _cnn_check(x, weights, B, F)
    for t, n, w in ((pool1, "pool1", CNN_POOL1 ** 2 * F), (pool2, "pool2", CNN_POOL2 ** 2 * F),
                    (feat, "feat", CNN_POOL2 ** 2 * F), (dF, "dF", CNN_POOL2 ** 2 * F)):
        _chk(t, n)
        if t.numel() != B * w:
            raise ValueError(f"{n} must hold {B} x {w} elements, got {t.numel()}")
    _chk(part, "part")
    if part.numel() < cnn_partial_elems(B, ipw):
        raise ValueError(f"part holds {part.numel()} elements, a batch of {B} needs "
                         f"{cnn_partial_elems(B, ipw)}")
    for g, w in zip(grads, weights):
        _chk(g, "grad")
        if g.shape != w.shape:
            raise ValueError(f"gradient of shape {tuple(g.shape)} for a tensor {tuple(w.shape)}")
    w1, b1, w2, b2, w3, _ = weights
    _ops.cnn_enc_backward_(x, w1, b1, w2, b2, w3, pool1, pool2, feat, dF, B, F, ipw, part,
                           *grads)


EVAL_CAP = 8      # boxes / loop steps per image of the metrics kernel (= evaluation.EVAL_CAP)
EVAL_COLUMNS = 25  # precision[11], recall[11], gt best-IoU, detection best-IoU, global IoU


def eval_detection(gt_boxes: torch.Tensor, gt_num: torch.Tensor, shifts: torch.Tensor,
                   scales: torch.Tensor, det_num: torch.Tensor, csize: float,
                   thresholds: torch.Tensor, per_image: torch.Tensor, offset: int = 0,
                   max_steps: Optional[int] = None) -> None:
    """Detection metrics of images [offset, offset + n) of a test set
    (mog_eval_detection): gt_boxes [N, G, 4] float64, gt_num [N] int32, shifts
    [n, steps, 2] and scales [n, steps] or [n, steps, 1] (float32 or float64,
    any image / step strides: the models' transposed views are read in place),
    det_num [n] int32, thresholds = evaluation.THRESHOLDS on the device ->
    per_image [N, 25] float64, rows [offset, offset + n).  Detections at or
    beyond `steps` are zero rows; det_num is clamped to max_steps (default
    `steps`).  G, max_steps <= 8."""
    _chk(gt_boxes, "gt_boxes", torch.float64)
    _chk(gt_num, "gt_num", torch.int32)
    _chk(per_image, "per_image", torch.float64)
    _chk(thresholds, "thresholds", torch.float64)
    _chk(det_num, "det_num", torch.int32)
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise ValueError(f"gt_boxes must be [N, G, 4], got {tuple(gt_boxes.shape)}")
    N, G = gt_boxes.shape[0], gt_boxes.shape[1]
    if shifts.dim() != 3 or shifts.shape[2] != 2:
        raise ValueError(f"shifts must be [n, steps, 2], got {tuple(shifts.shape)}")
    n, steps = shifts.shape[0], shifts.shape[1]
    T = steps if max_steps is None else int(max_steps)
    if not 1 <= G <= EVAL_CAP:
        raise ValueError(f"{G} ground-truth boxes per image: the kernel holds 1..{EVAL_CAP}")
    if T > EVAL_CAP or steps > T:
        raise ValueError(f"{steps} step rows of at most {T}: the kernel holds {EVAL_CAP} "
                         "and steps <= max_steps")
    if scales.dim() == 3 and scales.shape[2] == 1:
        scales = scales[:, :, 0]
    for t, name in ((shifts, "shifts"), (scales, "scales")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a HIP device tensor")
        if t.dtype not in (torch.float32, torch.float64) or t.dtype != shifts.dtype:
            raise ValueError(f"{name} must be float32 or float64 (both alike), got {t.dtype}")
    if tuple(scales.shape) != (n, steps):
        raise ValueError(f"scales must be [{n}, {steps}(, 1)], got {tuple(scales.shape)}")
    if steps and n and shifts.stride(2) != 1:
        raise ValueError("the two shift components must be adjacent in memory")
    if min(shifts.stride()[:2] + scales.stride()) < 0:
        raise ValueError("negative strides")
    if tuple(gt_num.shape) != (N,) or tuple(det_num.shape) != (n,):
        raise ValueError(f"gt_num must be [{N}] and det_num [{n}]")
    if tuple(per_image.shape) != (N, EVAL_COLUMNS) or thresholds.numel() != 11:
        raise ValueError(f"per_image must be [{N}, {EVAL_COLUMNS}] and thresholds hold 11 values")
    if offset < 0 or offset + n > N:
        raise ValueError(f"images [{offset}, {offset + n}) of a test set of {N}")
    _ops.eval_detection_(gt_boxes, gt_num, N, G, shifts, scales, shifts.stride(0),
                         shifts.stride(1), scales.stride(0), scales.stride(1), det_num, n, T,
                         steps, float(csize), thresholds, per_image, int(offset))


def eval_detection_means(per_image: torch.Tensor, means: torch.Tensor) -> None:
    """means [25] = the column means of per_image [N, 25] float64 in an order
    fixed by N (mog_eval_detection_means): the same bits on every run."""
    _chk(per_image, "per_image", torch.float64)
    _chk(means, "means", torch.float64)
    if per_image.dim() != 2 or per_image.shape[1] != EVAL_COLUMNS or per_image.shape[0] < 1:
        raise ValueError(f"per_image must be [N >= 1, {EVAL_COLUMNS}], got "
                         f"{tuple(per_image.shape)}")
    if means.numel() != EVAL_COLUMNS:
        raise ValueError(f"means must hold {EVAL_COLUMNS} values, got {means.numel()}")
    _ops.eval_detection_means_(per_image, per_image.shape[0], means)


ASR_NQ = 30        # record slots of asr_cell.hip (= asr_model.NQ)
ASR_LOG_T_MAX = 8  # loop steps the log-row kernel holds
# the AIR-ASR model's log variables, in the order of its ``log_variables``
ASR_LOG_NAMES = ("z_pres_kl", "scale_kl", "shift_kl", "vae_kl", "pr_num", "recon", "mse",
                 "area_loss", "out_loss", "size_loss", "over_loss", "num_margin", "num_min_KL",
                 "TotLoss", "elbo", "accu")


def asr_log_row(arec: torch.Tensor, vkl: torch.Tensor, zmask: torch.Tensor, live: torch.Tensor,
                bce: torch.Tensor, mse: torch.Tensor, area: torch.Tensor, outl: torch.Tensor,
                size: torch.Tensor, over: torch.Tensor, element: torch.Tensor,
                klsum: torch.Tensor, margin: torch.Tensor, means: torch.Tensor,
                out: torch.Tensor, slots: Sequence[int]) -> None:
    """out [16] = the AIR-ASR log row (ASR_LOG_NAMES) of the step whose
    workspace arrays are given, in one launch without a host read
    (mog_asr_log_row): arec [T, 30, B], vkl / zmask [T, B], live int32 [T] or
    [T + 1], bce .. klsum [B], margin [1], means [4]; ``slots``: the record
    slots (zkl, skl, shkl, prn) of arec.  Sums over the executed steps (the sum
    of live[:T]) and the batch in float64, in a fixed order.  1 <= T <= 8."""
    _chk(out, "out")
    if tuple(out.shape) != (len(ASR_LOG_NAMES),):
        raise ValueError(f"out must be [{len(ASR_LOG_NAMES)}], got {tuple(out.shape)}")
    _chk(arec, "arec")
    if arec.dim() != 3 or arec.shape[1] != ASR_NQ or arec.shape[2] < 1:
        raise ValueError(f"arec must be [T, {ASR_NQ}, B >= 1], got {tuple(arec.shape)}")
    T, B = arec.shape[0], arec.shape[2]
    if not 1 <= T <= ASR_LOG_T_MAX:
        raise ValueError(f"{T} loop steps: the kernel holds 1..{ASR_LOG_T_MAX}")
    _chk(live, "live", torch.int32)
    if live.dim() != 1 or live.shape[0] not in (T, T + 1):
        raise ValueError(f"live must be [{T}] or [{T + 1}], got {tuple(live.shape)}")
    for t, name, shape in ((vkl, "vkl", (T, B)), (zmask, "zmask", (T, B)), (bce, "bce", (B,)),
                           (mse, "mse", (B,)), (area, "area", (B,)), (outl, "outl", (B,)),
                           (size, "size", (B,)), (over, "over", (B,)),
                           (element, "element", (B,)), (klsum, "klsum", (B,)),
                           (margin, "margin", (1,)), (means, "means", (4,))):
        _chk(t, name)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {tuple(t.shape)}")
    for t, name in ((arec, "arec"), (vkl, "vkl"), (zmask, "zmask"), (live, "live"), (bce, "bce"),
                    (mse, "mse"), (area, "area"), (outl, "outl"), (size, "size"), (over, "over"),
                    (element, "element"), (klsum, "klsum"), (margin, "margin"), (means, "means")):
        if t.device != out.device:
            raise ValueError(f"{name} is on {t.device}, out on {out.device}")
    slots = [int(s) for s in slots]
    if len(slots) != 4 or not all(0 <= s < ASR_NQ for s in slots):
        raise ValueError(f"slots must be 4 record slots in [0, {ASR_NQ}), got {slots}")
    _ops.asr_log_row_(B, T, slots, arec, vkl, zmask, live, bce, mse, area, outl, size, over,
                      element, klsum, margin, means, out)


def gather_rows(src: torch.Tensor, idx, out: torch.Tensor, ksrc: Optional[torch.Tensor] = None,
                kout: Optional[torch.Tensor] = None) -> None:
    """out[b] = src[idx[b]] for the B picks of `idx` (and kout[b] =
    ksrc[idx[b]], int32, in the same launch; mog_gather_rows).  `idx`: a host
    sequence / array / CPU tensor of row numbers, checked against src's rows
    here (ValueError, no launch) and uploaded as int32.  Rows of `out` at or
    beyond B are left alone."""
    _chk(src, "src")
    _chk(out, "out")
    if src.dim() != 2 or out.dim() != 2 or out.shape[1] != src.shape[1]:
        raise ValueError(f"src [rows, width] and out [>= B, width], got {tuple(src.shape)} and "
                         f"{tuple(out.shape)}")
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        raise ValueError("idx must be on the host: it is range-checked before the launch")
    host = torch.as_tensor(idx).reshape(-1)
    if host.dtype.is_floating_point or host.dtype == torch.bool:
        raise ValueError(f"idx must be integers, got {host.dtype}")
    B, rows, width = host.numel(), src.shape[0], src.shape[1]
    if B and (int(host.min()) < 0 or int(host.max()) >= rows):
        raise ValueError(f"idx outside [0, {rows})")
    if out.shape[0] < B:
        raise ValueError(f"out holds {out.shape[0]} rows, idx picks {B}")
    if (ksrc is None) != (kout is None):
        raise ValueError("ksrc and kout go together")
    if ksrc is not None:
        _chk(ksrc, "ksrc", torch.int32)
        _chk(kout, "kout", torch.int32)
        if ksrc.numel() != rows or kout.numel() < B:
            raise ValueError(f"ksrc must hold {rows} values and kout at least {B}")
    dev_idx = host.to(torch.int32).to(src.device)
    _ops.gather_rows_(src, ksrc, dev_idx, rows, width, B, out, kout)


SUMM_NB, SUMM_NPOS, SUMM_NSTAT = 1551, 774, 6  # buckets, positive limits, stats columns
SUMM_CAP = 8  # loop steps / object counts of the grouped-means kernel (= EVAL_CAP)


def _same_device(ref: torch.Tensor, named) -> None:
    for t, name in named:
        if t.device != ref.device:
            raise ValueError(f"{name} is on {t.device}, the op on {ref.device}")


def summary_histograms(buf: torch.Tensor, t_off: torch.Tensor, t_len: torch.Tensor,
                       t_bt: torch.Tensor, t_bs: torch.Tensor, n_blocks: int,
                       thresholds: torch.Tensor, counts: torch.Tensor, stats: torch.Tensor,
                       work: torch.Tensor, sumsq: Optional[torch.Tensor] = None,
                       clip: Optional[float] = None,
                       denom: Optional[torch.Tensor] = None) -> None:
    """TensorFlow's default histogram and the moments of every variable of the
    flat fp32 buffer ``buf`` over the optimizer's table (ParamStore.t_off,
    t_len, t_bt, t_bs, n_blocks), in one call (mog_summ_hist): counts [V, 1551]
    int32 and stats [V, 6] float64 = (min, max, num, sum, sum_squares,
    nonfinite), both fully written.  ``thresholds`` [774] float32:
    summaries.bucket_thresholds() on the device; ``work``: float64 scratch of
    at least 6 * n_blocks.  Raw mode takes every value as it is.  Applied mode
    (``sumsq``, ``clip`` and ``denom`` together): sumsq [n_blocks] are the
    chunk sums the optimizer left, denom [V] float32 receives each tensor's
    max(norm, clip), and every value is (g * clip) / denom, the bits Adam
    consumed.  Everything is checked before the launch."""
    _chk(buf, "buf")
    _chk(counts, "counts", torch.int32)
    _chk(stats, "stats", torch.float64)
    _chk(work, "work", torch.float64)
    _chk(thresholds, "thresholds")
    _chk(t_off, "t_off", torch.int64)
    _chk(t_len, "t_len", torch.int64)
    _chk(t_bt, "t_bt", torch.int32)
    _chk(t_bs, "t_bs", torch.int64)
    if buf.dim() != 1:
        raise ValueError(f"buf must be a flat buffer, got {tuple(buf.shape)}")
    if t_off.dim() != 1 or t_off.shape != t_len.shape:
        raise ValueError("t_off and t_len must be [V] alike")
    V, n_blocks = t_off.shape[0], int(n_blocks)
    if n_blocks < 0 or tuple(t_bt.shape) != (n_blocks,) or tuple(t_bs.shape) != (n_blocks,):
        raise ValueError(f"t_bt and t_bs must be [{n_blocks}] (n_blocks), got "
                         f"{tuple(t_bt.shape)} and {tuple(t_bs.shape)}")
    if tuple(counts.shape) != (V, SUMM_NB) or tuple(stats.shape) != (V, SUMM_NSTAT):
        raise ValueError(f"counts must be [{V}, {SUMM_NB}] and stats [{V}, {SUMM_NSTAT}], got "
                         f"{tuple(counts.shape)} and {tuple(stats.shape)}")
    if tuple(thresholds.shape) != (SUMM_NPOS,):
        raise ValueError(f"thresholds must be [{SUMM_NPOS}], got {tuple(thresholds.shape)}")
    if work.numel() < 6 * n_blocks:
        raise ValueError(f"work holds {work.numel()} values, the call needs {6 * n_blocks}")
    named = [(t_off, "t_off"), (t_len, "t_len"), (t_bt, "t_bt"), (t_bs, "t_bs"),
             (thresholds, "thresholds"), (counts, "counts"), (stats, "stats"), (work, "work")]
    applied = sumsq is not None or clip is not None or denom is not None
    if applied:
        if sumsq is None or clip is None or denom is None:
            raise ValueError("applied mode takes sumsq, clip and denom together")
        _chk(sumsq, "sumsq")
        _chk(denom, "denom")
        if tuple(sumsq.shape) != (n_blocks,):
            raise ValueError(f"sumsq must be [{n_blocks}] (the table's n_blocks), got "
                             f"{tuple(sumsq.shape)}")
        if tuple(denom.shape) != (V,):
            raise ValueError(f"denom must be [{V}], got {tuple(denom.shape)}")
        if not float(clip) > 0.0:
            raise ValueError(f"clip must be positive, got {clip}")
        named += [(sumsq, "sumsq"), (denom, "denom")]
    _same_device(buf, named)
    _ops.summ_hist_(buf, t_off, t_len, t_bt, t_bs, n_blocks, V, thresholds, sumsq,
                    float(clip) if applied else 0.0, counts, stats, denom, work)


def summary_groups(target: torch.Tensor, steps: torch.Tensor, bce: torch.Tensor,
                   acc_b: torch.Tensor, loss_b: torch.Tensor, scale: torch.Tensor,
                   zprob: torch.Tensor, zkl: torch.Tensor, skl: torch.Tensor, shkl: torch.Tensor,
                   vkl: torch.Tensor, live: torch.Tensor, max_digits: int, acc: torch.Tensor,
                   accumulate: bool = False) -> None:
    """The grouped sums of the numeric summaries of one test chunk
    (mog_summ_groups): target / steps [B] int32, bce / acc_b / loss_b [B], the
    six records [Tmax, B], live int32 [Tmax] or [Tmax + 1] -> acc [4 + 6 Tmax,
    max_digits + 2, 2] float64 = (sum, count) per row and group (the object
    counts 0..max_digits, then all images), overwritten or, with
    ``accumulate``, added to.  Record rows at or beyond the executed steps (the
    sum of live[:Tmax], formed on the device) count as 0.0 and are not read.
    B >= 1, Tmax, max_digits <= 8."""
    _chk(acc, "acc", torch.float64)
    _chk(target, "target", torch.int32)
    _chk(steps, "steps", torch.int32)
    _chk(live, "live", torch.int32)
    if target.dim() != 1 or target.shape[0] < 1:
        raise ValueError(f"target must be [B >= 1], got {tuple(target.shape)}")
    B = target.shape[0]
    if scale.dim() != 2 or scale.shape[1] != B:
        raise ValueError(f"scale must be [Tmax, {B}], got {tuple(scale.shape)}")
    Tmax, max_digits = scale.shape[0], int(max_digits)
    if not 1 <= Tmax <= SUMM_CAP or not 0 <= max_digits <= SUMM_CAP:
        raise ValueError(f"{Tmax} loop steps, {max_digits} objects: the kernel holds 1..{SUMM_CAP} "
                         f"steps and 0..{SUMM_CAP} objects")
    named = [(target, "target"), (steps, "steps"), (live, "live")]
    for t, name, shape in ((steps, "steps", (B,)), (bce, "bce", (B,)), (acc_b, "acc_b", (B,)),
                           (loss_b, "loss_b", (B,)), (scale, "scale", (Tmax, B)),
                           (zprob, "zprob", (Tmax, B)), (zkl, "zkl", (Tmax, B)),
                           (skl, "skl", (Tmax, B)), (shkl, "shkl", (Tmax, B)),
                           (vkl, "vkl", (Tmax, B))):
        if name != "steps":
            _chk(t, name)
            named.append((t, name))
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {tuple(t.shape)}")
    if live.dim() != 1 or live.shape[0] not in (Tmax, Tmax + 1):
        raise ValueError(f"live must be [{Tmax}] or [{Tmax + 1}], got {tuple(live.shape)}")
    rows = 4 + 6 * Tmax
    if tuple(acc.shape) != (rows, max_digits + 2, 2):
        raise ValueError(f"acc must be [{rows}, {max_digits + 2}, 2], got {tuple(acc.shape)}")
    _same_device(acc, named)
    _ops.summ_groups_(target, steps, bce, acc_b, loss_b, scale, zprob, zkl, skl, shkl, vkl, live,
                      B, Tmax, max_digits, bool(accumulate), acc)


SYNTH_SIDE, SYNTH_GMAX, SYNTH_MAX_INDEX = 32, 8, 2 ** 52


class SynthBank:
    """A glyph bank for ``synth_canvases``, checked once on the host and held
    on the device: bank [G, 32, 32] float32 (glyphs top-left aligned, zero
    padded), sizes [G, 2] int32 (h, w) and the object counts to draw from,
    for canvases of ``canvas`` x ``canvas`` pixels.  Everything that bounds a
    loop or an address of the kernel is refused here (ValueError): a bank side
    other than 32, h or w outside 1..min(32, canvas), a canvas outside 32..64,
    a count outside 0..8, an empty bank or count list, wrongly typed or
    non-contiguous arrays."""

    def __init__(self, bank, sizes, counts, canvas: int, device):
        import numpy as np
        for a, name, dt in ((bank, "bank", np.float32), (sizes, "sizes", np.int32)):
            if not isinstance(a, np.ndarray) or a.dtype != dt:
                raise ValueError(f"{name} must be a host array of {np.dtype(dt).name}")
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name} must be contiguous")
        if bank.ndim != 3 or bank.shape[0] < 1 or bank.shape[1:] != (SYNTH_SIDE, SYNTH_SIDE):
            raise ValueError(f"bank must be [G >= 1, {SYNTH_SIDE}, {SYNTH_SIDE}], got "
                             f"{bank.shape}")
        if sizes.shape != (bank.shape[0], 2):
            raise ValueError(f"sizes must be [{bank.shape[0]}, 2], got {sizes.shape}")
        canvas = int(canvas)
        if not SYNTH_SIDE <= canvas <= 64:
            raise ValueError(f"canvas {canvas} outside {SYNTH_SIDE}..64")
        if sizes.min() < 1 or sizes.max() > min(SYNTH_SIDE, canvas):
            raise ValueError(f"glyph sides outside 1..{min(SYNTH_SIDE, canvas)}")
        counts = np.asarray(counts)
        if counts.ndim != 1 or counts.size < 1 or counts.dtype.kind not in "iu":
            raise ValueError("counts must be a non-empty list of integers")
        if counts.min() < 0 or counts.max() > SYNTH_GMAX:
            raise ValueError(f"object counts outside 0..{SYNTH_GMAX}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the bank lives on a HIP device")
        self.canvas, self.G = canvas, int(bank.shape[0])
        self.bank = torch.from_numpy(bank).to(dev)
        self.sizes = torch.from_numpy(sizes).to(dev)
        self.counts = torch.from_numpy(counts.astype(np.int32)).to(dev)


def synth_canvases(sbank: SynthBank, seed: int, first: int, images: torch.Tensor,
                   digits: torch.Tensor, objects: torch.Tensor, status: torch.Tensor) -> None:
    """Images first .. first + b - 1 of stream `seed` (mog_synth_canvases; b =
    the rows of `images`): images [b, C*C] float32, digits [b], objects
    [b, 8, 5] = (glyph, x, y, w, h), -1 past digits, and status [b], int32.
    One launch on the current stream, no host synchronisation.  A wrong shape,
    dtype or device, or an image number at or beyond 2^52, raises ValueError
    before any launch."""
    if not isinstance(sbank, SynthBank):
        raise ValueError("sbank must be an ops.SynthBank")
    _chk(images, "images")
    for t, name in ((digits, "digits"), (objects, "objects"), (status, "status")):
        _chk(t, name, torch.int32)
    C = sbank.canvas
    if images.dim() != 2 or images.shape[1] != C * C:
        raise ValueError(f"images must be [b, {C * C}], got {tuple(images.shape)}")
    b = images.shape[0]
    if tuple(digits.shape) != (b,) or tuple(status.shape) != (b,) or \
            tuple(objects.shape) != (b, SYNTH_GMAX, 5):
        raise ValueError(f"digits and status must be [{b}] and objects [{b}, {SYNTH_GMAX}, 5]")
    for t, name in ((images, "images"), (digits, "digits"), (objects, "objects"),
                    (status, "status")):
        if t.device != sbank.bank.device:
            raise ValueError(f"{name} is on {t.device}, the bank on {sbank.bank.device}")
    seed, first = int(seed), int(first)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an unsigned 64-bit integer")
    if first < 0 or first + b > SYNTH_MAX_INDEX:
        raise ValueError(f"images [{first}, {first + b}) outside [0, 2^52)")
    _ops.synth_canvases_(sbank.bank, sbank.sizes, sbank.G, sbank.counts, sbank.counts.numel(), C,
                         _i64(seed), first, b, images, digits, objects, status)


def _i64(v: int) -> int:
    """a 64-bit counter / seed as the signed int64 of an op schema's `int`"""
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def rng_fill(out: torch.Tensor, seed: int, offset: int, normal: bool) -> None:
    _chk(out, "out")
    _ops.rng_fill_(out, _i64(seed), _i64(offset), bool(normal))


def spin(ticks: int, device=None) -> None:
    """Hold the current stream for `ticks` of the 100 MHz wall clock (test
    instrument mog_spin of libmog_air_test.so)."""
    if ticks == 0:
        return
    rc = _lib.load_test().mog_spin(int(ticks), stream_ptr())
    if rc != 0:
        raise _lib.MogError(f"mog_spin failed ({rc})")


def lds_poison(bits: int = 0x7FC00000) -> None:
    """Fill every CU's LDS with a 32-bit pattern on the current stream (test
    instrument mog_lds_poison of libmog_air_test.so; default a quiet NaN)."""
    rc = _lib.load_test().mog_lds_poison(int(bits) & 0xFFFFFFFF, stream_ptr())
    if rc != 0:
        raise _lib.MogError(f"mog_lds_poison failed ({rc})")


# function ids of mog_math_probe (include/mog_air_test.h); 0..6 are the
# oracle's oracle_math_vec ids
PROBE_FNS = ("exp", "log", "expm1", "tanh", "sigmoid", "softplus", "log1p", "logistic_noise",
             "lse0", "concrete_kl", "gauss_kl_term", "chain_dot", "chain64")
_PROBE_NARGS = (1, 1, 1, 1, 1, 1, 1, 1, 1, 5, 6, 2, 2)


def math_probe(fn, *args: torch.Tensor, K: int = 0, ldw: int = 1) -> torch.Tensor:
    """One function of include/mog_math.h / csrc/step_math.h as the device
    compiler builds it, over arrays of arguments (test instrument
    mog_math_probe of libmog_air_test.so).  `fn`: an id or a name of
    PROBE_FNS.  Elementwise functions take equally long fp32 vectors.  The
    chains take a [n, K] and w (K rows of pitch ldw; column 0 is read) and
    return the n k-ordered fma chains."""
    fn = PROBE_FNS.index(fn) if isinstance(fn, str) else int(fn)
    if not 0 <= fn < len(PROBE_FNS) or len(args) != _PROBE_NARGS[fn]:
        raise ValueError(f"math_probe: function {fn} takes {_PROBE_NARGS[fn]} arrays")
    for j, t in enumerate(args):
        _chk(t, f"args[{j}]")
    if PROBE_FNS[fn] in ("chain_dot", "chain64"):
        a, w = args
        if PROBE_FNS[fn] == "chain64":
            K = 64
        if a.dim() != 2 or a.shape[1] != K or K < 0 or ldw < 1:
            raise ValueError("math_probe: a must be [n, K], ldw >= 1")
        if w.numel() < (0 if K == 0 else (K - 1) * ldw + 1):
            raise ValueError("math_probe: w holds fewer than (K - 1) ldw + 1 elements")
        n = a.shape[0]
    else:
        n = args[0].numel()
        if any(t.numel() != n for t in args):
            raise ValueError("math_probe: argument arrays differ in length")
    y = torch.empty(n, device=args[0].device, dtype=torch.float32)
    if n == 0:
        return y
    # (K == 0: a and w hold nothing and have null data_ptrs; never read)
    ptrs = _lib.ptr_array([t.data_ptr() or y.data_ptr() for t in args])
    rc = _lib.load_test().mog_math_probe(fn, ptrs, len(args), y.data_ptr(), n, int(K), int(ldw),
                                         stream_ptr())
    if rc != 0:
        raise _lib.MogError(f"mog_math_probe failed ({rc})")
    return y
