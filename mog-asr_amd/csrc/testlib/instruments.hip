// Test-only instruments (include/mog_air_test.h), built into
// mog_air/_lib/libmog_air_test.so -- not part of the product library.
//
// mog_spin: one wave that occupies `stream` for a wall-clock interval.
// tests/test_gpu_streams.py launches it at the head of one stream of a forked
// train step, so that a cross-stream dependency the host code forgot (a fork
// without its wait, a join without its event, a buffer the other stream still
// reads) turns from a rare timing accident into a failure on every run.
//
// mog_lds_poison: every CU's LDS filled with one pattern before a kernel, so
// that a read of LDS the kernel did not write first shows in its outputs.
//
// mog_math_probe: the device compilation of include/mog_math.h and
// csrc/step_math.h, one function per launch over arrays of arguments, so that
// tests/test_gpu_math_spec.py can compare its bits with the oracle's (gcc's)
// at the functions' edges.  It calls the header functions as they are.
#include "../mog_common.h"
#include "../step_math.h"
#include "../../../include/mog_air_test.h"

namespace {

__global__ __launch_bounds__(64) void spin_kernel(long long ticks) {
  // wall_clock64: the constant 100 MHz counter; the wave sleeps between
  // polls.  ticks is capped by the host (<= 1 s), so every wave exits.
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// Fills the LDS of every CU with one 32-bit pattern (a NaN, say): run before
// a kernel, it makes any read of LDS that the kernel did not write first show
// up in its outputs instead of depending on what ran there before.
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned bits) {
  extern __shared__ unsigned lds_words[];
  constexpr int WORDS = 80 * 1024 / 4;
  for (int i = threadIdx.x; i < WORDS; i += 256)
    __hip_atomic_store(&lds_words[i], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
}

struct ProbeArgs {
  const float* a[6];
};

// one thread per element, plain loads and stores
__global__ __launch_bounds__(256) void math_probe_kernel(int fn, ProbeArgs p, float* y, long n,
                                                         int K, int ldw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r;
  switch (fn) {
    case MOG_PROBE_EXP: r = mog_expf(p.a[0][i]); break;
    case MOG_PROBE_LOG: r = mog_logf(p.a[0][i]); break;
    case MOG_PROBE_EXPM1: r = mog_expm1f(p.a[0][i]); break;
    case MOG_PROBE_TANH: r = mog_tanhf(p.a[0][i]); break;
    case MOG_PROBE_SIGMOID: r = mog_sigmoidf(p.a[0][i]); break;
    case MOG_PROBE_SOFTPLUS: r = mog_softplusf(p.a[0][i]); break;
    case MOG_PROBE_LOG1P: r = mog_log1pf(p.a[0][i]); break;
    case MOG_PROBE_LOGISTIC_NOISE: r = logistic_noise(p.a[0][i]); break;
    case MOG_PROBE_LSE0: r = lse0(p.a[0][i]); break;
    case MOG_PROBE_CONCRETE_KL:
      r = concrete_kl(p.a[0][i], p.a[1][i], p.a[2][i], p.a[3][i], p.a[4][i]);
      break;
    case MOG_PROBE_GAUSS_KL_TERM:
      r = gauss_kl_term(p.a[0][i], p.a[1][i], p.a[2][i], p.a[3][i], p.a[4][i], p.a[5][i]);
      break;
    case MOG_PROBE_CHAIN_DOT: r = chain_dot(p.a[0] + (size_t)i * K, p.a[1], K, ldw); break;
    default: r = chain64(p.a[0] + (size_t)i * 64, p.a[1], ldw); break;  // MOG_PROBE_CHAIN64
  }
  y[i] = r;
}

}  // namespace

extern "C" int mog_math_probe(int fn, const float* const* args, int nargs, float* y, long n,
                              int K, int ldw, void* stream) {
  static const int want[MOG_PROBE_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 5, 6, 2, 2};
  MOG_CHECK_ARG(fn >= 0 && fn < MOG_PROBE_COUNT && args && nargs == want[fn] && y && n >= 0);
  const bool chain = fn == MOG_PROBE_CHAIN_DOT || fn == MOG_PROBE_CHAIN64;
  MOG_CHECK_ARG(!chain || (K >= 0 && ldw >= 1 && (fn != MOG_PROBE_CHAIN64 || K == 64)));
  ProbeArgs p{};
  for (int j = 0; j < nargs; ++j) {
    MOG_CHECK_ARG(args[j] != nullptr);
    p.a[j] = args[j];
  }
  if (n == 0) return 0;
  math_probe_kernel<<<mog_cdiv(n, 256), 256, 0, mog_stream(stream)>>>(fn, p, y, n, K, ldw);
  MOG_LAUNCH_RET();
}

extern "C" int mog_lds_poison(unsigned bits, void* stream) {
  // 80 KiB per workgroup (two fill a CU's 160 KiB), eight rounds of them
  lds_poison_kernel<<<256 * 2 * 8, 256, 80 * 1024, mog_stream(stream)>>>(bits);
  MOG_LAUNCH_RET();
}

extern "C" int mog_spin(long long ticks, void* stream) {
  MOG_CHECK_ARG(ticks >= 0 && ticks <= 100000000LL);
  if (ticks == 0) return 0;
  spin_kernel<<<1, 64, 0, mog_stream(stream)>>>(ticks);
  MOG_LAUNCH_RET();
}
