// Device numerics the loop-step kernels share (air_cell.hip, asr_cell.hip,
// asr_gen.hip): k-ordered fma chains, the concrete distribution's noise and
// KL, the Gaussian KL term.  Each is held bit-exact against the oracle
// (oracle/air_ref.c, oracle/asr_ref.c): one rounding per operation
// (contraction off in every function), mog_math.h transcendentals.
#pragma once
#include "mog_common.h"

// sum_k a[k] w[k ldw] as ONE fma chain in k order (the oracle's dense()).
// The operands of 32 k-steps are loaded before their fmas: a rolled
// load-then-fma loop paid one memory round trip per k (16 us per launch at
// the reference's batch of 64, where the step kernel is one or two
// workgroups); same fma sequence, same bits.
__device__ __forceinline__ float chain_dot(const float* a, const float* w, int K, int ldw) {
#pragma clang fp contract(off)
  constexpr int KB = 32;
  float acc = 0.0f;
  int k = 0;
  for (; k + KB <= K; k += KB) {
    float av[KB], wv[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      av[i] = a[k + i];
      wv[i] = w[(size_t)(k + i) * ldw];
    }
#pragma unroll
    for (int i = 0; i < KB; ++i) acc = fmaf(av[i], wv[i], acc);
  }
  for (; k < K; ++k) acc = fmaf(a[k], w[(size_t)k * ldw], acc);
  return acc;
}

// the same chain over AIR-ASR's 64 hidden units (a compile-time K)
__device__ __forceinline__ float chain64(const float* a, const float* w, int ldw) {
#pragma clang fp contract(off)
  float acc = 0.0f;
#pragma unroll
  for (int k0 = 0; k0 < 64; k0 += 32) {
    float av[32], wv[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      av[i] = a[k0 + i];
      wv[i] = w[(size_t)(k0 + i) * ldw];
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) acc = fmaf(av[i], wv[i], acc);
  }
  return acc;
}

// logistic noise of the concrete z_pres sample from u ~ U(0, 1)
// (concrete.py:20-27)
__device__ __forceinline__ float logistic_noise(float u) {
#pragma clang fp contract(off)
  const float eps = 1e-9f;
  return mog_logf(u + eps) - mog_logf((1.0f - u) + eps);
}

__device__ __forceinline__ float lse0(float a) {
#pragma clang fp contract(off)
  float m = a > 0.0f ? a : 0.0f;
  if (!(m - m == 0.0f)) m = 0.0f;
  return mog_logf(mog_expf(0.0f - m) + mog_expf(a - m)) + m;
}

// KL of two concrete distributions at the sample y (concrete.py:30-64)
__device__ __forceinline__ float concrete_kl(float y, float plo, float pT, float qlo, float qT) {
#pragma clang fp contract(off)
  const float eps = 1e-9f;
  const float lse_p = lse0(-y * pT + plo);
  const float log_prior = ((mog_logf(pT + eps) - y * (pT + 1.0f)) + plo) - 2.0f * lse_p;
  const float lse_q = lse0(-y * qT + qlo);
  const float log_post = ((mog_logf(qT + eps) - y * (qT + 1.0f)) + qlo) - 2.0f * lse_q;
  return log_post - log_prior;
}

__device__ __forceinline__ float gauss_kl_term(float plv, float lv, float var, float pv,
                                               float mean, float pm) {
#pragma clang fp contract(off)
  const float d = mean - pm;
  return (((plv - lv) - 1.0f) + var / pv) + (d * d) / pv;
}
