// The reference's TensorBoard summaries, reduced where the data lies
// (air/air_model.py:216-264, 896-993).
//
// mog_summ_hist: TensorFlow's default histogram (1551 buckets, limits
// +-1e-12 * 1.1^k, 0 and +-DBL_MAX) and the moments of every variable of a
// flat fp32 buffer, walked by the optimizer's own table (optim.hip: one block
// per 4096-element chunk).  Three launches:
//   init    counts = 0, stats = (DBL_MAX, -DBL_MAX, 0, 0, 0, 0), denom = clip
//   chunk   each block classifies its chunk into an LDS histogram, adds the
//           non-empty bins to counts with integer atomics (order independent)
//           and leaves its chunk's (sum, sum_squares, min, max, num,
//           nonfinite) in `work`
//   finish  one thread per tensor adds the tensor's chunk partials in chunk
//           order
// so two calls on the same input give the same bits.  Classification: a
// bucket's index is the number of limits <= x.  No limit is an fp32 value, so
// the table `thr` (774 floats, thr[k] = the smallest fp32 above limit k, from
// the caller, compared and never recomputed) decides exactly: c = the number
// of thr[k] <= |x| by binary search in LDS, bucket = 776 + c for x >= 0 and
// 775 - c below.  Applied mode rebuilds what clip_adam_kernel consumed: the
// tensor's squared norm from the optimizer's chunk sums in the same order, the
// same sqrtf / fmaxf, and (g * clip) / denom without contraction.
//
// mog_summ_groups: the numeric summaries' grouped sums of one test chunk, one
// block per row, every sum in a fixed order in double.
#include <float.h>

#include "mog_common.h"

extern "C" int mog_optim_chunk_elems(void);

namespace {

constexpr int CHUNK = 4096;  // = mog_optim_chunk_elems(), checked at launch
constexpr int NPOS = 774;    // positive limits below DBL_MAX
constexpr int NB = 2 * NPOS + 3;
constexpr int NSTAT = 6;     // min, max, num, sum, sum_squares, nonfinite
constexpr int NWORK = 6;     // sum, sum_squares, min, max, num, nonfinite

__global__ __launch_bounds__(256) void summ_init_kernel(unsigned* counts, double* stats,
                                                       float* denom, int V, float clip) {
  const long n = (long)V * NB;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    counts[i] = 0u;
  if (blockIdx.x == 0)
    for (int v = threadIdx.x; v < V; v += 256) {
      double* s = stats + (long)v * NSTAT;
      s[0] = DBL_MAX;
      s[1] = -DBL_MAX;
      s[2] = s[3] = s[4] = s[5] = 0.0;
      if (denom != nullptr) denom[v] = clip;  // a tensor without elements: norm 0
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

template <bool APPLIED>
__global__ __launch_bounds__(256) void summ_hist_kernel(
    const float* __restrict__ buf, long total, const long* __restrict__ off,
    const long* __restrict__ len, const int* __restrict__ block_tensor,
    const long* __restrict__ block_start, int nblocks, int V, const float* __restrict__ thr,
    const float* __restrict__ part, float clip, unsigned* __restrict__ counts,
    float* __restrict__ denom_out, double* __restrict__ work) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[NB];
  __shared__ float sthr[NPOS];
  __shared__ float red[4];
  __shared__ double dred[6][4];
  const int tid = threadIdx.x;
  for (int b = tid; b < NB; b += 256) hist[b] = 0u;
  for (int k = tid; k < NPOS; k += 256) sthr[k] = thr[k];
  // the table's entries, clamped so that nothing they hold leaves the buffer
  const int ti = min(max(block_tensor[blockIdx.x], 0), V - 1);
  const long base = min(max(off[ti], 0L), total);
  const long n = min(max(len[ti], 0L), total - base);
  const long c0 = min(max(block_start[blockIdx.x], 0L), n);
  const long c1 = min(n, c0 + CHUNK);

  float denom = 1.0f;
  if (APPLIED) {
    // clip_adam_kernel's norm (optim.hip): the tensor's chunk sums, blocks
    // first .. first + nc - 1, per thread strided, then the block tree
    int first = blockIdx.x - (int)(c0 / CHUNK);
    int nc = (int)((n + CHUNK - 1) / CHUNK);
    first = max(first, 0);
    nc = min(nc, nblocks - first);
    float s = 0.0f;
    for (int j = tid; j < nc; j += 256) s += part[first + j];
    const float l2 = mog_block_sum256(s, red);
    const float norm = l2 > 0.0f ? sqrtf(l2) : l2;
    denom = fmaxf(norm, clip);
    if (c0 == 0 && tid == 0) denom_out[ti] = denom;
  }
  __syncthreads();

  double sum = 0.0, sq = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
  unsigned num = 0u, bad = 0u;
  auto take = [&](float g) {
    const float x = APPLIED ? (g * clip) / denom : g;
    const float a = fabsf(x);
    if (!(a <= FLT_MAX)) {  // NaN, +-Inf: counted, not added
      ++bad;
      return;
    }
    // c = the number of thresholds <= a (thr ascending)
    int lo = 0, hi = NPOS;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sthr[mid] <= a) lo = mid + 1;
      else hi = mid;
    }
    // -0.0 goes with +0.0 (0.0 <= -0.0): the sign of the value, not of its bit
    const int b = x < 0.0f ? NPOS + 1 - lo : NPOS + 2 + lo;
    atomicAdd(&hist[min(max(b, 0), NB - 1)], 1u);
    const double d = (double)x;
    sum += d;
    sq += d * d;
    mn = fmin(mn, d);
    mx = fmax(mx, d);
    ++num;
  };
  const float* p = buf + base;
  // 16-byte reads where the tensor starts on one (the parameter store aligns
  // every tensor to 64 elements), the ragged end element by element
  const bool vec = ((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  const long v1 = vec ? c0 + ((c1 - c0) & ~3L) : c0;
  for (long i = c0 + 4 * tid; i < v1; i += 1024) {
    const float4 g4 = *reinterpret_cast<const float4*>(p + i);
    take(g4.x);
    take(g4.y);
    take(g4.z);
    take(g4.w);
  }
  for (long i = v1 + tid; i < c1; i += 256) take(p[i]);
  __syncthreads();
  unsigned* out = counts + (long)ti * NB;
  for (int b = tid; b < NB; b += 256)
    if (hist[b] != 0u) atomicAdd(out + b, hist[b]);

  // the chunk's partials: lanes, then the four waves, in a fixed order
  const double r0 = wave_sum_d(sum), r1 = wave_sum_d(sq), r2 = wave_min_d(mn),
               r3 = wave_max_d(mx), r4 = wave_sum_d((double)num), r5 = wave_sum_d((double)bad);
  const int w = tid >> 6, l = tid & 63;
  if (l == 0) {
    dred[0][w] = r0;
    dred[1][w] = r1;
    dred[2][w] = r2;
    dred[3][w] = r3;
    dred[4][w] = r4;
    dred[5][w] = r5;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = work + (long)blockIdx.x * NWORK;
    o[0] = (dred[0][0] + dred[0][1]) + (dred[0][2] + dred[0][3]);
    o[1] = (dred[1][0] + dred[1][1]) + (dred[1][2] + dred[1][3]);
    o[2] = fmin(fmin(dred[2][0], dred[2][1]), fmin(dred[2][2], dred[2][3]));
    o[3] = fmax(fmax(dred[3][0], dred[3][1]), fmax(dred[3][2], dred[3][3]));
    o[4] = (dred[4][0] + dred[4][1]) + (dred[4][2] + dred[4][3]);
    o[5] = (dred[5][0] + dred[5][1]) + (dred[5][2] + dred[5][3]);
  }
}

// one thread per block of the table; the thread of a tensor's first block
// adds the tensor's chunks in chunk order
__global__ __launch_bounds__(256) void summ_finish_kernel(const long* __restrict__ len,
                                                         const int* __restrict__ block_tensor,
                                                         const long* __restrict__ block_start,
                                                         int nblocks, int V,
                                                         const double* __restrict__ work,
                                                         double* __restrict__ stats) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks || block_start[b] != 0) return;
  const int ti = min(max(block_tensor[b], 0), V - 1);
  const long n = max(len[ti], 0L);
  const int nc = (int)min((long)(nblocks - b), (n + CHUNK - 1) / CHUNK);
  double sum = 0.0, sq = 0.0, mn = DBL_MAX, mx = -DBL_MAX, num = 0.0, bad = 0.0;
  for (int j = 0; j < nc; ++j) {
    const double* w = work + (long)(b + j) * NWORK;
    sum += w[0];
    sq += w[1];
    mn = fmin(mn, w[2]);
    mx = fmax(mx, w[3]);
    num += w[4];
    bad += w[5];
  }
  double* s = stats + (long)ti * NSTAT;
  s[0] = mn;
  s[1] = mx;
  s[2] = num;
  s[3] = sum;
  s[4] = sq;
  s[5] = bad;
}

// ------------------------------------------------------- grouped means ----
constexpr int GCAP = 8;        // Tmax <= 8, max_digits <= 8
constexpr int NG = GCAP + 2;   // groups 0..max_digits and "all"

// row r: 0 steps, 1 rec_loss, 2 digit_acc, 3 total_loss; 4 + q * Tmax + i:
// step i of record q (scale, z_pres_prob, z_pres_kl, scale_kl, shift_kl, vae_kl)
__global__ __launch_bounds__(256) void summ_groups_kernel(
    const int* __restrict__ target, const int* __restrict__ steps, const float* __restrict__ bce,
    const float* __restrict__ acc_b, const float* __restrict__ loss_b,
    const float* __restrict__ scale, const float* __restrict__ zprob,
    const float* __restrict__ zkl, const float* __restrict__ skl, const float* __restrict__ shkl,
    const float* __restrict__ vkl, const int* __restrict__ live, int B, int Tmax, int max_digits,
    int accumulate, double* __restrict__ acc) {
#pragma clang fp contract(off)
  __shared__ double rs[NG][4], rc[NG][4];
  const int r = blockIdx.x, tid = threadIdx.x;
  int T = 0;
  for (int t = 0; t < Tmax; ++t) T += live[t];  // executed loop steps
  T = min(max(T, 0), Tmax);
  int q = -1, i = 0;
  const float* src = nullptr;
  if (r == 1) src = bce;
  else if (r == 2) src = acc_b;
  else if (r == 3) src = loss_b;
  else if (r >= 4) {
    q = (r - 4) / Tmax;
    i = (r - 4) % Tmax;
    const float* rec = q == 0 ? scale : q == 1 ? zprob : q == 2 ? zkl : q == 3 ? skl
                       : q == 4 ? shkl : vkl;
    // rows at or beyond T are the reference's zero padding: never read
    src = i < T ? rec + (long)i * B : nullptr;
  }
  // steps > i (scale and the KLs of a step the image took), steps > i - 1
  // (z_pres_kl: one more step), no mask (z_pres_prob and the per-image rows)
  const bool masked = q >= 0 && q != 1;
  const int need = q == 2 ? i - 1 : i;
  double s[NG], c[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) s[g] = c[g] = 0.0;
  for (int b = tid; b < B; b += 256) {
    const int st = steps[b];
    if (masked && !(st > need)) continue;
    const double v = r == 0 ? (double)(float)st : src != nullptr ? (double)src[b] : 0.0;
    const int tg = target[b];
#pragma unroll
    for (int g = 0; g < NG - 1; ++g)
      if (tg == g && g <= max_digits) {
        s[g] += v;
        c[g] += 1.0;
      }
    s[NG - 1] += v;
    c[NG - 1] += 1.0;
  }
  const int w = tid >> 6, l = tid & 63;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const double a = wave_sum_d(s[g]), n = wave_sum_d(c[g]);
    if (l == 0) {
      rs[g][w] = a;
      rc[g][w] = n;
    }
  }
  __syncthreads();
  // groups 0..max_digits, then "all" as group max_digits + 1
  if (tid <= max_digits + 1) {
    const int g = tid <= max_digits ? tid : NG - 1;
    const double a = (rs[g][0] + rs[g][1]) + (rs[g][2] + rs[g][3]);
    const double n = (rc[g][0] + rc[g][1]) + (rc[g][2] + rc[g][3]);
    double* o = acc + ((long)r * (max_digits + 2) + tid) * 2;
    if (accumulate) {
      o[0] += a;
      o[1] += n;
    } else {
      o[0] = a;
      o[1] = n;
    }
  }
}

}  // namespace

extern "C" int mog_summ_hist(const float* buf, long total, const long* off, const long* len,
                             const int* block_tensor, const long* block_start, int nblocks,
                             int ntensors, const float* thresholds, const float* sumsq,
                             float clip, unsigned int* counts, double* stats, float* denom,
                             double* work, void* stream) {
  MOG_CHECK_ARG(mog_optim_chunk_elems() == CHUNK);
  MOG_CHECK_ARG(nblocks >= 0 && ntensors >= 0 && total >= 0);
  if (ntensors == 0) return 0;
  MOG_CHECK_ARG(counts && stats);
  const bool applied = sumsq != nullptr;
  MOG_CHECK_ARG(!applied || (denom != nullptr && clip > 0.0f));
  hipStream_t s = mog_stream(stream);
  const unsigned zb = min(mog_cdiv((long)ntensors * NB, 256), 1024u);
  summ_init_kernel<<<zb, 256, 0, s>>>(counts, stats, applied ? denom : nullptr, ntensors, clip);
  if (nblocks > 0) {
    MOG_CHECK_ARG(buf && off && len && block_tensor && block_start && thresholds && work);
    if (applied)
      summ_hist_kernel<true><<<nblocks, 256, 0, s>>>(buf, total, off, len, block_tensor,
                                                     block_start, nblocks, ntensors, thresholds,
                                                     sumsq, clip, counts, denom, work);
    else
      summ_hist_kernel<false><<<nblocks, 256, 0, s>>>(buf, total, off, len, block_tensor,
                                                      block_start, nblocks, ntensors, thresholds,
                                                      nullptr, 0.0f, counts, nullptr, work);
    summ_finish_kernel<<<mog_cdiv(nblocks, 256), 256, 0, s>>>(len, block_tensor, block_start,
                                                              nblocks, ntensors, work, stats);
  }
  MOG_LAUNCH_RET();
}

extern "C" int mog_summ_groups(const int* target, const int* steps, const float* bce,
                               const float* acc_b, const float* loss_b, const float* scale,
                               const float* zprob, const float* zkl, const float* skl,
                               const float* shkl, const float* vkl, const int* live, int B,
                               int Tmax, int max_digits, int accumulate, double* acc,
                               void* stream) {
  MOG_CHECK_ARG(B >= 1 && Tmax >= 1 && Tmax <= GCAP && max_digits >= 0 && max_digits <= GCAP);
  MOG_CHECK_ARG(target && steps && bce && acc_b && loss_b && scale && zprob && zkl && skl &&
                shkl && vkl && live && acc);
  summ_groups_kernel<<<4 + 6 * Tmax, 256, 0, mog_stream(stream)>>>(
      target, steps, bce, acc_b, loss_b, scale, zprob, zkl, skl, shkl, vkl, live, B, Tmax,
      max_digits, accumulate, acc);
  MOG_LAUNCH_RET();
}
