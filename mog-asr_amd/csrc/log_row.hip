// The AIR-ASR model's log row on the device (include/mog_air.h,
// mog_asr_log_row): the 16 scalars of
// asr_model.AIRModel.log_variables from the step's workspace arrays in one
// launch, so that a trainer can keep every step's row in a device buffer and
// read it when a log line is due.
//
// One 1024-thread workgroup, like batch_mean_kernel (air_cell.hip): the work
// is (5 T_exec + 9) B floats, a latency-bound reduction.  Thread i owns the
// images b = i, i + 1024, ...; for each it issues every load of the image
// (5 T_exec record values, 9 per-image values) before the first add, then adds
// them to 13 float64 accumulators in step order.  The accumulators are summed
// over the wave by xor shuffles and over the 16 waves in wave order: the order
// depends on (B, T_exec) alone, there is no atomic, and two launches on equal
// inputs give equal bits.  Each sum is divided by B in float64 and rounded
// once to fp32.  Rows t >= T_exec are never loaded.
#include "mog_common.h"

namespace {

constexpr int NT = 1024, NW = NT / MOG_WAVE, TMAX = 8;
constexpr int NSUM = 13;  // 4 record slots, vae_kl, 7 per-image arrays, elbo

// out[] position of sum k, in log_variables' order; positions 11 (num_margin),
// 13 (TotLoss) and 15 (accu) are copies
__constant__ const int OUT_OF_SUM[NSUM] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 9, 10, 12, 14};

struct LogRowArgs {
  const float* arec;  // [T][NQ][B]
  const float* vkl;   // [T][B]
  const float* zmask;  // [T][B]
  const int* live;    // [>= T]
  const float* per[7];  // bce, mse, area, outl, size, over, element [B]
  const float* klsum;   // [B]
  const float* margin;  // [1]
  const float* means;   // [>= 2]
  int q[4];             // record slots zkl, skl, shkl, prn
  int NQ, T, B;
  float* out;  // [16]
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NT) void asr_log_row_kernel(LogRowArgs a) {
  __shared__ double red[NSUM][NW];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int T = a.T, B = a.B;
  // the executed steps, as Results._T() counts them (clamped: no row past T)
  int Tx = 0;
  for (int t = 0; t < T; ++t) Tx += a.live[t];
  Tx = min(max(Tx, 0), T);

  double acc[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;

  for (int b = tid; b < B; b += NT) {
    float r[4][TMAX], vm[TMAX], p[7], e;
    // every load of this image in flight before the first add
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < Tx) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k][t] = a.arec[((long)t * a.NQ + a.q[k]) * B + b];
        vm[t] = a.vkl[(long)t * B + b] * a.zmask[(long)t * B + b];  // fp32, as the property forms it
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = a.per[k][b];
    e = a.klsum[b] + p[0];  // fp32 sum klsum + bce
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < Tx) {
        acc[0] += (double)r[0][t];
        acc[1] += (double)r[1][t];
        acc[2] += (double)r[2][t];
        acc[3] += (double)r[3][t];
        acc[4] += (double)vm[t];
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[5 + k] += (double)p[k];
    acc[12] += (double)e;
  }

#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const double s = wave_sum_f64(acc[k]);
    if (l == 0) red[k][w] = s;
  }
  __syncthreads();
  if (tid < NSUM) {
    double s = red[tid][0];
#pragma unroll
    for (int i = 1; i < NW; ++i) s += red[tid][i];
    a.out[OUT_OF_SUM[tid]] = (float)(s / (double)B);
  } else if (tid < 16) {
    // the copied entries keep their bits
    const unsigned* src = reinterpret_cast<const unsigned*>(
        tid == 13 ? a.margin : (tid == 14 ? a.means : a.means + 1));
    reinterpret_cast<unsigned*>(a.out)[tid == 13 ? 11 : (tid == 14 ? 13 : 15)] = *src;
  }
}

}  // namespace

extern "C" int mog_asr_log_row(const float* arec, int NQ, const int* q, const float* vkl,
                               const float* zmask, const int* live, const float* bce,
                               const float* mse, const float* area, const float* outl,
                               const float* size, const float* over, const float* element,
                               const float* klsum, const float* margin, const float* means, int T,
                               int B, float* out, void* stream) {
  MOG_CHECK_ARG(T >= 1 && T <= TMAX && B >= 1 && NQ >= 1 && q);
  MOG_CHECK_ARG(arec && vkl && zmask && live && bce && mse && area && outl && size && over &&
                element && klsum && margin && means && out);
  LogRowArgs a;
  for (int k = 0; k < 4; ++k) {
    MOG_CHECK_ARG(q[k] >= 0 && q[k] < NQ);
    a.q[k] = q[k];
  }
  a.arec = arec;
  a.vkl = vkl;
  a.zmask = zmask;
  a.live = live;
  const float* per[7] = {bce, mse, area, outl, size, over, element};
  for (int k = 0; k < 7; ++k) a.per[k] = per[k];
  a.klsum = klsum;
  a.margin = margin;
  a.means = means;
  a.NQ = NQ;
  a.T = T;
  a.B = B;
  a.out = out;
  hipLaunchKernelGGL(asr_log_row_kernel, dim3(1), dim3(NT), 0, mog_stream(stream), a);
  MOG_LAUNCH_RET();
}
