// Detection metrics of a whole test set on the device:
// mog_air/evaluation.py:42-78 restated for every image at once, in float64.
//
// Arithmetic contract: every IoU is the bits the host computes -- one IEEE
// double rounding per operation in the host's order, no contraction (this
// object is built with -ffp-contract=off, mog-asr_amd/Makefile, and the
// arithmetic below also carries the pragma), IEEE division.  The thresholds
// come from the caller (the float64 values of evaluation.THRESHOLDS); they
// are never recomputed here.
//
// Structure: the work per image is tiny and latency-bound.  Eight lanes share
// one image (16 images per 128-thread workgroup): lane l builds detection l's
// box and its IoU column, then gt row l's maximum; the IoU matrix and the
// assignment's subset table live in LDS (no per-thread array is indexed
// dynamically, so nothing goes to scratch).  The optimal assignment is a
// dynamic programme over subsets of the larger side: best[mask] = the largest
// summed IoU of the first popcount(mask) rows of the smaller side matched to
// the columns in mask; layer p (popcount p) reads only layer p - 1, and the
// eight lanes of an image split each layer's masks.
#include "mog_common.h"

namespace {

constexpr int CAP = 8;           // G <= 8, T <= 8
constexpr int LANES = 8;         // lanes per image
constexpr int IMGS = 16;         // images per workgroup
constexpr int NT = IMGS * LANES;  // 128
constexpr int NTHR = 11, NCOL = 25;

struct ImageLds {
  double iou[CAP][CAP];      // [gt][det]
  double best[1 << CAP];     // subset table of the assignment
  double rowmax[CAP], colmax[CAP];
};

// np.add.reduce of n <= 8 contiguous doubles: sequential below 8, numpy's
// unrolled pairwise block at 8
__device__ __forceinline__ double np_sum8(const double* a, int n) {
#pragma clang fp contract(off)
  if (n == 8) return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  double r = 0.0;
  for (int i = 0; i < n; ++i) r += a[i];
  return r;
}

template <typename T>
__global__ __launch_bounds__(NT) void eval_det_kernel(
    const double* __restrict__ gt_boxes, const int* __restrict__ gt_num, int G,
    const T* __restrict__ shifts, const T* __restrict__ scales, long sh_img, long sh_step,
    long sc_img, long sc_step, const int* __restrict__ det_num, int n, int Tcap, int steps,
    double csize, const double* __restrict__ thr, double* __restrict__ per_image, int offset) {
#pragma clang fp contract(off)
  __shared__ ImageLds lds[IMGS];
  __shared__ double sthr[NTHR];
  const int slot = threadIdx.x / LANES, l = threadIdx.x % LANES;
  const int i = blockIdx.x * IMGS + slot;  // image of this chunk
  const bool on = i < n;
  ImageLds& L = lds[slot];
  if (threadIdx.x < NTHR) sthr[threadIdx.x] = thr[threadIdx.x];

  int ng = 0, nd = 0;
  if (on) {
    ng = min(max(gt_num[offset + i], 0), G);
    nd = min(max(det_num[i], 0), Tcap);
  }
  // detection l's box; rows at or beyond `steps` read as zero
  double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0, area_d = 0.0;
  if (on && l < nd) {
    double sx = 0.0, sy = 0.0, s = 0.0;
    if (l < steps) {
      const T* sh = shifts + (long)i * sh_img + (long)l * sh_step;
      sx = (double)sh[0];
      sy = (double)sh[1];
      s = (double)scales[(long)i * sc_img + (long)l * sc_step];
    }
    const double half = csize / 2;
    const double cx = (sx + 1) * half, cy = (sy + 1) * half, r = s * half;
    d0 = cx - r;
    d1 = cy - r;
    d2 = cx + r;
    d3 = cy + r;
    area_d = ((d2 - d0) + 1) * ((d3 - d1) + 1);
  }
  // column l of the IoU matrix and its maximum
  if (on && l < nd) {
    double cm = 0.0;
    for (int g = 0; g < ng; ++g) {
      const double* gb = gt_boxes + ((long)(offset + i) * G + g) * 4;
      const double g0 = gb[0], g1 = gb[1], g2 = gb[2], g3 = gb[3];
      const double xa = fmax(g0, d0), ya = fmax(g1, d1);
      const double xb = fmin(g2, d2), yb = fmin(g3, d3);
      const double inter = fmax(0.0, (xb - xa) + 1) * fmax(0.0, (yb - ya) + 1);
      const double area_g = ((g2 - g0) + 1) * ((g3 - g1) + 1);
      const double v = inter / ((area_g + area_d) - inter);
      L.iou[g][l] = v;
      cm = g == 0 ? v : fmax(cm, v);
    }
    L.colmax[l] = cm;
  }
  if (l == 0) L.best[0] = 0.0;
  __syncthreads();
  if (on && l < ng && nd > 0) {
    double rm = L.iou[l][0];
    for (int d = 1; d < nd; ++d) rm = fmax(rm, L.iou[l][d]);
    L.rowmax[l] = rm;
  }
  // the assignment: rows = the smaller side, columns = the larger
  const bool gt_rows = ng <= nd;
  const int K = gt_rows ? ng : nd, M = gt_rows ? nd : ng;
  for (int p = 1; p <= CAP; ++p) {
    if (on && p <= K) {
      for (int mask = l; mask < (1 << M); mask += LANES) {
        if (__popc((unsigned)mask) != p) continue;
        double b = -1.0;  // below every sum of IoUs
        for (int j = 0; j < M; ++j) {
          if (!((mask >> j) & 1)) continue;
          const double w = gt_rows ? L.iou[p - 1][j] : L.iou[j][p - 1];
          b = fmax(b, L.best[mask ^ (1 << j)] + w);
        }
        L.best[mask] = b;
      }
    }
    __syncthreads();
  }
  if (!on) return;
  // columns l, l + 8, l + 16, l + 24 of this image's row
  double* out = per_image + (long)(offset + i) * NCOL;
  for (int c = l; c < NCOL; c += LANES) {
    double v;
    if (ng == 0 && nd == 0) {
      v = 1.0;
    } else if (ng == 0) {
      v = c >= NTHR && c < 2 * NTHR ? 1.0 : 0.0;
    } else if (nd == 0) {
      v = 0.0;
    } else if (c < 2 * NTHR) {
      const double t = sthr[c < NTHR ? c : c - NTHR];
      int hit = 0;
      for (int d = 0; d < nd; ++d) hit += L.colmax[d] > t ? 1 : 0;
      v = (double)hit / (double)(c < NTHR ? nd : ng);
    } else if (c == 2 * NTHR) {
      v = np_sum8(L.rowmax, ng) / (double)ng;
    } else if (c == 2 * NTHR + 1) {
      v = np_sum8(L.colmax, nd) / (double)nd;
    } else {
      double b = -1.0;
      for (int mask = 0; mask < (1 << M); ++mask)
        if (__popc((unsigned)mask) == K) b = fmax(b, L.best[mask]);
      v = b / (double)max(nd, ng);
    }
    out[c] = v;
  }
}

// means[c] = sum over rows of per_image[:, c] / N in an order that depends on
// N alone: 32 row segments summed in row order, the segments added in order
constexpr int MSEG = 32, MNT = MSEG * 32;

__global__ __launch_bounds__(MNT) void eval_det_means_kernel(const double* __restrict__ per_image,
                                                             int N, double* __restrict__ means) {
#pragma clang fp contract(off)
  __shared__ double red[MSEG][32];
  const int c = threadIdx.x & 31, s = threadIdx.x >> 5;
  const int per = (N + MSEG - 1) / MSEG;
  double acc = 0.0;
  if (c < NCOL)
    for (int r = s * per; r < min(N, (s + 1) * per); ++r) acc += per_image[(long)r * NCOL + c];
  red[s][c] = acc;
  __syncthreads();
  if (s == 0 && c < NCOL) {
    double v = red[0][c];
    for (int k = 1; k < MSEG; ++k) v += red[k][c];
    means[c] = v / (double)N;
  }
}

}  // namespace

extern "C" int mog_eval_detection(const double* gt_boxes, const int* gt_num, int G,
                                  const void* shifts, const void* scales, int f64,
                                  long shift_image_stride, long shift_step_stride,
                                  long scale_image_stride, long scale_step_stride,
                                  const int* det_num, int n, int T, int steps, double csize,
                                  const double* thresholds, double* per_image, int offset,
                                  void* stream) {
  MOG_CHECK_ARG(n >= 0 && offset >= 0 && G >= 1 && G <= CAP && T >= 0 && T <= CAP);
  MOG_CHECK_ARG(steps >= 0 && steps <= T && csize > 0.0);
  if (n == 0) return 0;
  MOG_CHECK_ARG(gt_boxes && gt_num && det_num && thresholds && per_image);
  MOG_CHECK_ARG(steps == 0 || (shifts && scales));
  const dim3 grid(mog_cdiv(n, IMGS)), block(NT);
  hipStream_t s = mog_stream(stream);
  if (f64)
    hipLaunchKernelGGL(eval_det_kernel<double>, grid, block, 0, s, gt_boxes, gt_num, G,
                       static_cast<const double*>(shifts), static_cast<const double*>(scales),
                       shift_image_stride, shift_step_stride, scale_image_stride,
                       scale_step_stride, det_num, n, T, steps, csize, thresholds, per_image,
                       offset);
  else
    hipLaunchKernelGGL(eval_det_kernel<float>, grid, block, 0, s, gt_boxes, gt_num, G,
                       static_cast<const float*>(shifts), static_cast<const float*>(scales),
                       shift_image_stride, shift_step_stride, scale_image_stride,
                       scale_step_stride, det_num, n, T, steps, csize, thresholds, per_image,
                       offset);
  MOG_LAUNCH_RET();
}

extern "C" int mog_eval_detection_means(const double* per_image, int N, double* means,
                                        void* stream) {
  MOG_CHECK_ARG(N >= 1 && per_image && means);
  hipLaunchKernelGGL(eval_det_means_kernel, dim3(1), dim3(MNT), 0, mog_stream(stream),
                     per_image, N, means);
  MOG_LAUNCH_RET();
}
