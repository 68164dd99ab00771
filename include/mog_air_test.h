/* Test-only instruments (mog-asr_amd/csrc/testlib/instruments.hip, built into
 * mog_air/_lib/libmog_air_test.so; not part of the product library
 * libmog_air.so).  Loaded by mog_air.ops.spin / lds_poison for the
 * stream-ordering and LDS-hygiene tests (tests/test_gpu_streams.py,
 * scripts/stn_concurrency.py) and by mog_air.ops.math_probe for the
 * device-bits-equal-host-bits test (tests/test_gpu_math_spec.py). */
#ifndef MOG_AIR_TEST_H
#define MOG_AIR_TEST_H
#ifdef __cplusplus
extern "C" {
#endif

/* One wave occupying `stream` for `ticks` of the 100 MHz wall clock (<= 1 s):
 * the stream-ordering tests hold one stream of a forked step back with it. */
int mog_spin(long long ticks, void* stream);
/* Fills the LDS of every CU with the 32-bit pattern `bits` (a NaN, say), so a
 * kernel launched next that reads LDS it did not write shows it. */
int mog_lds_poison(unsigned bits, void* stream);

/* y[i] = f(args[0][i], ..) for i < n, f one function of include/mog_math.h or
 * csrc/step_math.h as the device compiler builds it (one thread per element).
 * `args`: a host array of `nargs` device pointers, each of n floats.  Ids 0..6
 * are oracle_math_vec's.  The chains: element i is the k-ordered fma chain of
 * row i of args[0] ([n, K] row-major) with column 0 of args[1] (K rows, pitch
 * ldw); chain64 takes K == 64.  K and ldw are ignored by the other ids. */
enum {
  MOG_PROBE_EXP = 0,
  MOG_PROBE_LOG,
  MOG_PROBE_EXPM1,
  MOG_PROBE_TANH,
  MOG_PROBE_SIGMOID,
  MOG_PROBE_SOFTPLUS,
  MOG_PROBE_LOG1P,
  MOG_PROBE_LOGISTIC_NOISE, /* (u) */
  MOG_PROBE_LSE0,           /* (a) */
  MOG_PROBE_CONCRETE_KL,    /* (y, prior log-odds, prior T, posterior log-odds, posterior T) */
  MOG_PROBE_GAUSS_KL_TERM,  /* (prior log-var, log-var, var, prior var, mean, prior mean) */
  MOG_PROBE_CHAIN_DOT,      /* (a, w) */
  MOG_PROBE_CHAIN64,        /* (a, w) */
  MOG_PROBE_COUNT
};
int mog_math_probe(int fn, const float* const* args, int nargs, float* y, long n, int K, int ldw,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOG_AIR_TEST_H */
