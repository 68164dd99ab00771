// AIR-ASR generation (second half):
// air/air_number_bbox_location.py:1124-1361 and vae.py:51-86.  Per loop step,
// around the generative LSTMCell / decoder GEMMs and the STN write the model
// already has: the gen_shift output chains and prior draws, the constant
// write scale, the z_pres prior (fixed or learned) with its rounded concrete
// sample, stopping sum, counts and live flag (asr_gen_step_kernel), and the
// binarisation of the decoded window (bernoulli_threshold_kernel).  fp32, one
// rounding per operation (contraction off), k-ordered fma chains, mog_math.h
// transcendentals: the numerics of asr_cell.hip.
#include "mog_common.h"
#include "step_math.h"

namespace {

constexpr int HS = 64;  // hidden units of every head (step_math.h chain64)

struct GenCfg {
  int G, Z, step, fix_steps;
  float thr, temperature, scale_prior_mean, scale_prior_var, s, vae_prior_mean, vae_prior_logvar;
};

struct GenIO {
  const float* hid_m;      // [G,64] relu(gen_shift/dense(hg))
  const float* hid_v;      // [G,64] relu(gen_shift/dense_2(hg))
  const float* hid_p;      // [G,64] relu(z_pres/prior/dense(hg_prev)), null with fix_steps >= 0
  const float* w[6];       // gen_shift dense_1 W,b [64,2], dense_3 W,b; z_pres prior dense_1 W,b
  const float* eps_shift;  // [G,2]
  const float* eps_scale;  // [G]
  const float* eps_z;      // [G,Z]
  const float* u;          // [G]
  float* stop;             // [G] state
  int* digits;             // [G] state
  int* live;               // [T+1]
  float* ss;               // [G,3] shift latent x, y; scale latent
  float* z;                // [G,Z]
  float* theta_back;       // [G,6]
  float* zval;             // [G]
  float* zmask;            // [G]
  // learned scale prior (null with the fixed one)
  const float* hid_gm;     // [G,64] gen_scale/dense chain over hg (raw: no latent terms / bias)
  const float* hid_gv;     // [G,64] gen_scale/dense_2 likewise
  const float* gw[8];      // gen_scale dense W,b [258,64], dense_1 W,b [66,1], dense_2, dense_3
};

// One wave per image (4 per block), as asr_step_fwd_kernel: lanes 0..4 run the
// five output-layer chains, every lane draws its latent elements, lane 0
// finishes the image.  LearnedScale (fix_scale_distribution=False,
// :1170-1201): every lane finishes its unit of the two gen_scale hidden layers
// on the generated shift latent, lanes 0 / 1 run the output chains, and the
// scale latent is drawn from that Gaussian.
template <bool LearnedScale>
__global__ __launch_bounds__(256) void asr_gen_step_kernel(GenCfg cfg, GenIO io) {
#pragma clang fp contract(off)
  __shared__ float sv[4][8];
  __shared__ float sh8[LearnedScale ? 4 : 1][HS], sh9[LearnedScale ? 4 : 1][HS];
  const int m = threadIdx.x >> 6, q = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + m;
  const bool ok = g < cfg.G;
  const int gc = ok ? g : 0;  // clamped image index: loads only, no store
  const int Z = cfg.Z;
  // every per-image input before the first store (stores through possibly
  // aliasing pointers would order each later load behind them)
  const float es0 = io.eps_shift[(size_t)gc * 2], es1 = io.eps_shift[(size_t)gc * 2 + 1];
  const float e_s = io.eps_scale[gc], uu = io.u[gc], stop_old = io.stop[gc];
  const int dig = io.digits[gc];
  const float ez = q < Z ? io.eps_z[(size_t)gc * Z + q] : 0.0f;
  float h8 = 0.0f, h9 = 0.0f, w8a = 0.0f, w8b = 0.0f, b8 = 0.0f, w9a = 0.0f, w9b = 0.0f, b9 = 0.0f;
  if constexpr (LearnedScale) {
    const size_t rq = (size_t)gc * HS + q;
    h8 = io.hid_gm[rq]; h9 = io.hid_gv[rq];
    w8a = io.gw[0][256 * HS + q]; w8b = io.gw[0][257 * HS + q]; b8 = io.gw[1][q];
    w9a = io.gw[4][256 * HS + q]; w9b = io.gw[4][257 * HS + q]; b9 = io.gw[5][q];
  }
  if (q < 5) {
    const size_t r = (size_t)gc * HS;
    float v;
    switch (q) {
      case 0: v = chain64(io.hid_m + r, io.w[0], 2) + io.w[1][0]; break;
      case 1: v = chain64(io.hid_m + r, io.w[0] + 1, 2) + io.w[1][1]; break;
      case 2: v = chain64(io.hid_v + r, io.w[2], 2) + io.w[3][0]; break;
      case 3: v = chain64(io.hid_v + r, io.w[2] + 1, 2) + io.w[3][1]; break;
      default:
        v = cfg.fix_steps >= 0 ? (cfg.step < cfg.fix_steps ? 100.0f : -100.0f)
                               : chain64(io.hid_p + r, io.w[4], 1) + io.w[5][0];
    }
    sv[m][q] = v;
  }
  __syncthreads();
  float gcm = 0.0f, gclv = 0.0f;
  if constexpr (LearnedScale) {
    // every lane the shift latent (the same bits), then its hidden unit
    const float l0 = sv[m][0] + es0 * sqrtf(mog_expf(sv[m][2]));
    const float l1 = sv[m][1] + es1 * sqrtf(mog_expf(sv[m][3]));
    float a8 = h8, a9 = h9;
    a8 = fmaf(l0, w8a, a8);
    a8 = fmaf(l1, w8b, a8);
    a8 = a8 + b8;
    a9 = fmaf(l0, w9a, a9);
    a9 = fmaf(l1, w9b, a9);
    a9 = a9 + b9;
    sh8[m][q] = a8 > 0.0f ? a8 : 0.0f;
    sh9[m][q] = a9 > 0.0f ? a9 : 0.0f;
    __syncthreads();
    if (q < 2) {
      const float* hh = q == 0 ? sh8[m] : sh9[m];
      const float* w = io.gw[q == 0 ? 2 : 6];
      float acc = chain64(hh, w, 1);
      acc = fmaf(l0, w[HS], acc);
      acc = fmaf(l1, w[HS + 1], acc);
      sv[m][5 + q] = acc + io.gw[q == 0 ? 3 : 7][0];
    }
    __syncthreads();
    gcm = sv[m][5];
    gclv = sv[m][6];
  }
  if (!ok) return;
  // latent (vae.py:63-66): every lane its elements
  const float zsd = sqrtf(mog_expf(cfg.vae_prior_logvar));
  if (q < Z) io.z[(size_t)g * Z + q] = cfg.vae_prior_mean + ez * zsd;
  for (int k = q + 64; k < Z; k += 64)
    io.z[(size_t)g * Z + k] = cfg.vae_prior_mean + io.eps_z[(size_t)g * Z + k] * zsd;
  if (q != 0) return;
  // shift latent and the fixed-prior scale latent (:1156-1201); the scale the
  // transform uses is the constant s (:1203-1205)
  const float sl0 = sv[m][0] + es0 * sqrtf(mog_expf(sv[m][2]));
  const float sl1 = sv[m][1] + es1 * sqrtf(mog_expf(sv[m][3]));
  const float tx = mog_tanhf(sl0), ty = mog_tanhf(sl1);
  float cl = cfg.scale_prior_mean + e_s * sqrtf(cfg.scale_prior_var);
  if constexpr (LearnedScale) cl = gcm + e_s * sqrtf(mog_expf(gclv));
  const float s = cfg.s;
  float* tb = io.theta_back + (size_t)g * 6;
  tb[0] = 1.0f / s; tb[1] = 0.0f; tb[2] = -tx / s; tb[3] = 0.0f; tb[4] = 1.0f / s; tb[5] = -ty / s;
  io.ss[(size_t)g * 3] = sl0;
  io.ss[(size_t)g * 3 + 1] = sl1;
  io.ss[(size_t)g * 3 + 2] = cl;
  // z_pres: concrete sample at the prior log-odds, always rounded (:1259-1285)
  const float noise = logistic_noise(uu);
  const float y = (sv[m][4] + noise) / cfg.temperature;
  const float zp = rintf(mog_sigmoidf(y));
  // stopping sum, counts, canvas mask (:1287-1303)
  const float stop_new = stop_old + (1.0f - zp);
  io.stop[g] = stop_new;
  const bool act = stop_new < cfg.thr;
  if (act) {
    io.digits[g] = dig + 1;
    io.live[cfg.step + 1] = 1;
  }
  io.zval[g] = zp;
  io.zmask[g] = act ? 1.0f : 0.0f;
}

// out[i] = x[i] > u[i] ? 1 : 0 (relu(sign(x - u)), vae.py:83-84): threads
// below n4 take one float4 each, the rest one element of the tail from 4 * n4
// (out may be x or u: each element is read and written by one thread)
__global__ __launch_bounds__(256) void bernoulli_threshold_kernel(const float* x, const float* u,
                                                                  float* out, long n4, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) {
    const floatx4 a = reinterpret_cast<const floatx4*>(x)[i];
    const floatx4 b = reinterpret_cast<const floatx4*>(u)[i];
    floatx4 r;
    r.x = a.x > b.x ? 1.0f : 0.0f;
    r.y = a.y > b.y ? 1.0f : 0.0f;
    r.z = a.z > b.z ? 1.0f : 0.0f;
    r.w = a.w > b.w ? 1.0f : 0.0f;
    reinterpret_cast<floatx4*>(out)[i] = r;
    return;
  }
  const long j = 4 * n4 + (i - n4);
  if (j < n) out[j] = x[j] > u[j] ? 1.0f : 0.0f;
}

}  // namespace

// gw == null: the fixed scale prior; else gw[8] / ghid[2] of the learned one,
// which reads no constant prior: the kernel config then holds N(0, 1)
// whatever the caller passed
extern "C" int mog_asr_gen_step(int G, int Z, int step, int fix_steps, float thr,
                                float temperature, float scale_prior_mean, float scale_prior_var,
                                float s, float vae_prior_mean, float vae_prior_logvar,
                                const float* const* w, const float* const* hid,
                                const float* const* gw, const float* const* ghid,
                                const float* eps_shift, const float* eps_scale,
                                const float* eps_z, const float* u, float* stop, int* digits,
                                int* live, float* ss, float* z, float* theta_back, float* zval,
                                float* zmask, void* stream) {
  MOG_CHECK_ARG(G >= 0 && Z > 0 && step >= 0 && s > 0.0f && w && hid && eps_shift && eps_scale && eps_z && u);
  MOG_CHECK_ARG(stop && digits && live && ss && z && theta_back && zval && zmask);
  MOG_CHECK_ARG(hid[0] && hid[1] && (hid[2] || fix_steps >= 0));
  if (G == 0) return 0;
  GenCfg c{G, Z, step, fix_steps, thr, temperature, gw ? 0.0f : scale_prior_mean,
           gw ? 1.0f : scale_prior_var, s, vae_prior_mean, vae_prior_logvar};
  GenIO io{};
  io.hid_m = hid[0]; io.hid_v = hid[1]; io.hid_p = fix_steps >= 0 ? nullptr : hid[2];
  for (int i = 0; i < 6; ++i) {
    MOG_CHECK_ARG(w[i] || (i >= 4 && fix_steps >= 0));
    io.w[i] = w[i];
  }
  io.eps_shift = eps_shift; io.eps_scale = eps_scale; io.eps_z = eps_z; io.u = u;
  io.stop = stop; io.digits = digits; io.live = live; io.ss = ss; io.z = z;
  io.theta_back = theta_back; io.zval = zval; io.zmask = zmask;
  if (gw) {
    MOG_CHECK_ARG(ghid && ghid[0] && ghid[1]);
    io.hid_gm = ghid[0]; io.hid_gv = ghid[1];
    for (int i = 0; i < 8; ++i) {
      MOG_CHECK_ARG(gw[i]);
      io.gw[i] = gw[i];
    }
    asr_gen_step_kernel<true><<<mog_cdiv(G, 4), 256, 0, mog_stream(stream)>>>(c, io);
  } else {
    asr_gen_step_kernel<false><<<mog_cdiv(G, 4), 256, 0, mog_stream(stream)>>>(c, io);
  }
  MOG_LAUNCH_RET();
}

extern "C" int mog_bernoulli_threshold(const float* x, const float* u, float* out, long n,
                                       void* stream) {
  MOG_CHECK_ARG(x && u && out && n >= 0);
  if (n == 0) return 0;
  // float4 form only when all three rows are 16-byte aligned
  const bool al = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(u) |
                    reinterpret_cast<size_t>(out)) & 15) == 0;
  const long n4 = al ? n / 4 : 0;
  bernoulli_threshold_kernel<<<mog_cdiv(n4 + (n - 4 * n4), 256), 256, 0, mog_stream(stream)>>>(
      x, u, out, n4, n);
  MOG_LAUNCH_RET();
}
