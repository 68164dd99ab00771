// The cnn=True image encoder of the AIR model (air/air_model.py:763-810):
//   x [B, 50, 50, 1] -> conv1 5x5 same, 1 -> F, bias, relu      [B, 50, 50, F]
//                    -> max-pool 2x2 stride 2 valid              [B, 25, 25, F]
//                    -> conv2 5x5 same, F -> F, bias, relu       [B, 25, 25, F]
//                    -> max-pool 2x2 stride 2 valid              [B, 12, 12, F]
//                    -> conv3 5x5 same, F -> F, bias, relu       [B, 12, 12, F]
//   rnn_input = reshape(conv3, [B, 144 F])  (NHWC: feature (y 12 + x) F + f)
// with F = 8 (the reference default, the only width built), kernels HWIO.
//
// Arithmetic conventions (pinned by tests/test_gpu_air_cnn.py):
//  * forward: every conv output is ONE fp32 fmaf chain started at +0 over
//    (ky, kx, cin), cin fastest, then one add of the bias, then relu -- the
//    dense layers' convention (oracle/air_ref.c dense), so the forward is
//    bit-exact against im2col + that chain.  `same` padding is a two-pixel
//    zero border of the planes staged in LDS: a padded tap multiplies the
//    zero, exactly as im2col does, and no tap ever indexes outside a plane.
//  * pool2 reads conv2 rows / columns 0..23 only: row and column 24 take part
//    in no maximum, are never computed and receive no gradient.
//  * max-pool ties: the gradient goes to the FIRST maximum in row-major window
//    order (0,0), (0,1), (1,0), (1,1) (a strict > comparison): TF's CPU kernel
//    and torch.nn.functional.max_pool2d.
//  * relu gradient: dy (y > 0).
//  * weight / bias gradients: workgroup g owns images [g n, (g+1) n), sums
//    them in image order in registers and stores its partial sums; a second
//    launch adds the workgroups' partials in slices of consecutive workgroups,
//    each in index order, then the slices in order.  No atomics: the same bits
//    on every run of one batch size and one n.  n (images per workgroup) is
//    the caller's, by default B / 512 clamped to 1..8: one image per workgroup
//    up to a batch of 1023 (the reference's batch of 64 would otherwise walk
//    its images serially on 8 of the 256 CUs), 8 from 4096 (1024 workgroups
//    and 14 MB of partial sums at B = 8192).
//
// Stored by the forward for the backward: pool1 (25 25 F), pool2 (12 12 F) and
// the features, 5000 + 1152 + 1152 floats = 29,216 bytes per image.  The
// pre-pool planes of conv1 and conv2 (80,000 + 20,000 bytes per image) are not
// stored: the backward recomputes each 2x2 window (with the forward's own
// code, so the argmax and the relu mask are the forward's) -- 1.5 M of the
// backward's MACs per image -- and the weight gradients of conv1 / conv2 then
// read only the one argmax tap of each window.
//
// LDS (static, 256 threads = 4 waves per workgroup): forward 46,768 bytes
// (x 54x54, pool1 29x29xF, pool2 16x16xF, all zero-bordered), backward
// 45,472 bytes (three regions reused along the phases, see the kernel): three
// workgroups per CU by LDS (160 KiB), 12 of its 32 wave slots; the backward's
// 216 VGPRs allow two.  Weights are read through wave-uniform addresses (the
// scalar cache), not staged.
#include "mog_common.h"

namespace {

constexpr int F = 8;                // channels
constexpr int C = 50;               // canvas side
constexpr int XP = C + 4;           // zero-bordered canvas side
constexpr int S1 = 25, S1P = S1 + 4;  // pool1 side, zero-bordered
constexpr int S2 = 12, S2P = S2 + 4;  // pool2 / conv3 side, zero-bordered
constexpr int N1 = S1 * S1;         // 625 pool1 positions = conv1 windows
constexpr int N2 = S2 * S2;         // 144 pool2 positions = conv2 windows
constexpr int NF = N2 * F;          // 1152 features
constexpr int KW1 = 25 * F;         // conv1 kernel elements (200)
constexpr int KW2 = 25 * F * F;     // conv2 / conv3 kernel elements (1600)
// one workgroup's partial sums: [w1 | b1 | w2 | b2 | w3 | b3]
constexpr int OFF_W1 = 0, OFF_B1 = KW1, OFF_W2 = OFF_B1 + F, OFF_B2 = OFF_W2 + KW2;
constexpr int OFF_W3 = OFF_B2 + F, OFF_B3 = OFF_W3 + KW2, PART = OFF_B3 + F;  // 3424
constexpr int MAX_IPW = 8;          // most images per workgroup of the backward
constexpr int NT = 256;
constexpr int WJ = (KW2 + NT - 1) / NT;  // conv2 / conv3 kernel elements per thread (7)
constexpr int CH1 = 6, CH1_WIN = 105;    // conv1 weight gradient: 6 chunks of 105 windows

__device__ __forceinline__ float relu(float v) { return v > 0.0f ? v : 0.0f; }

// x [50, 50] -> xp [54, 54] with a zero border of 2
__device__ __forceinline__ void load_x(float* xp, const float* __restrict__ x, int t) {
  for (int i = t; i < XP * XP; i += NT) {
    const int y = i / XP - 2, xx = i % XP - 2;
    xp[i] = (y >= 0 && y < C && xx >= 0 && xx < C) ? x[y * C + xx] : 0.0f;
  }
}

// src [n, n, F] -> dst [n + 4, n + 4, F] with a zero border of 2
__device__ __forceinline__ void load_plane(float* dst, const float* __restrict__ src, int n,
                                           int t) {
  const int np = n + 4;
  floatx4* d4 = reinterpret_cast<floatx4*>(dst);
  const floatx4* s4 = reinterpret_cast<const floatx4*>(src);
  for (int i = t; i < np * np * 2; i += NT) {
    const int pos = i >> 1, y = pos / np - 2, x = pos % np - 2;
    floatx4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (y >= 0 && y < n && x >= 0 && x < n) v = s4[(y * n + x) * 2 + (i & 1)];
    d4[i] = v;
  }
}

__device__ __forceinline__ void load8(const float* p, float* v) {
  const floatx4 lo = reinterpret_cast<const floatx4*>(p)[0];
  const floatx4 hi = reinterpret_cast<const floatx4*>(p)[1];
  v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w;
  v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
}

// The four conv1 outputs (before the bias) of pooling window (wy, wx), all F
// channels: acc[dy 2 + dx][co], each one chain over (ky, kx).
__device__ __forceinline__ void conv1_window(const float* xp, const float* __restrict__ w1,
                                             int wy, int wx, float (*acc)[F]) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int co = 0; co < F; ++co) acc[d][co] = 0.0f;
  for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 5; ++kx) {
      const float* w = w1 + (ky * 5 + kx) * F;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float a = xp[(2 * wy + (d >> 1) + ky) * XP + 2 * wx + (d & 1) + kx];
#pragma unroll
        for (int co = 0; co < F; ++co) acc[d][co] = fmaf(a, w[co], acc[d][co]);
      }
    }
  }
}

// The four conv2 outputs (before the bias) of pooling window (wy, wx) for
// channels co0, co0 + 1 (co0 wave-uniform): acc[dy 2 + dx][j], each one chain
// over (ky, kx, ci).  a1: the zero-bordered pool1 plane.
__device__ __forceinline__ void conv2_window(const float* a1, const float* __restrict__ w2,
                                             int wy, int wx, int co0, float (*acc)[2]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) acc[d][0] = acc[d][1] = 0.0f;
  for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 5; ++kx) {
      const float* w = w2 + (ky * 5 + kx) * F * F + co0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float in[F];
        load8(a1 + ((2 * wy + (d >> 1) + ky) * S1P + 2 * wx + (d & 1) + kx) * F, in);
#pragma unroll
        for (int ci = 0; ci < F; ++ci) {
          acc[d][0] = fmaf(in[ci], w[ci * F], acc[d][0]);
          acc[d][1] = fmaf(in[ci], w[ci * F + 1], acc[d][1]);
        }
      }
    }
  }
}

// relu(bias-added) maximum of a window's four values and the index of its
// first maximum (row-major, strict >)
__device__ __forceinline__ float pool_first_max(float v0, float v1, float v2, float v3,
                                                float bias, int* arg) {
  float best = relu(v0 + bias);
  int a = 0;
  const float r1 = relu(v1 + bias), r2 = relu(v2 + bias), r3 = relu(v3 + bias);
  if (r1 > best) best = r1, a = 1;
  if (r2 > best) best = r2, a = 2;
  if (r3 > best) best = r3, a = 3;
  *arg = a;
  return best;
}

__global__ __launch_bounds__(NT) void cnn_enc_forward_kernel(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pool1, float* __restrict__ pool2,
    float* __restrict__ feat) {
  __shared__ __attribute__((aligned(16))) float xp[XP * XP];
  __shared__ __attribute__((aligned(16))) float a1[S1P * S1P * F];
  __shared__ __attribute__((aligned(16))) float a2[S2P * S2P * F];
  const int t = threadIdx.x, lane = t & 63;
  const int co0 = 2 * __builtin_amdgcn_readfirstlane(t >> 6);
  const size_t b = blockIdx.x;  // one image per workgroup (grid = B)
  load_x(xp, x + b * (C * C), t);
  for (int i = t; i < S1P * S1P * F; i += NT) a1[i] = 0.0f;
  for (int i = t; i < S2P * S2P * F; i += NT) a2[i] = 0.0f;
  __syncthreads();
  // conv1 + relu + pool1: a thread per window, all channels
  for (int win = t; win < N1; win += NT) {
    const int wy = win / S1, wx = win % S1;
    float acc[4][F];
    conv1_window(xp, w1, wy, wx, acc);
    float out[F];
#pragma unroll
    for (int co = 0; co < F; ++co) {
      int arg;
      out[co] = pool_first_max(acc[0][co], acc[1][co], acc[2][co], acc[3][co], b1[co], &arg);
    }
    float* dl = a1 + ((wy + 2) * S1P + wx + 2) * F;
    float* dg = pool1 + b * (N1 * F) + win * F;
#pragma unroll
    for (int co = 0; co < F; ++co) dl[co] = out[co], dg[co] = out[co];
  }
  __syncthreads();
  // conv2 + relu + pool2: a wave per channel pair, a lane per window
  for (int win = lane; win < N2; win += 64) {
    const int wy = win / S2, wx = win % S2;
    float acc[4][2];
    conv2_window(a1, w2, wy, wx, co0, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int arg;
      const float v = pool_first_max(acc[0][j], acc[1][j], acc[2][j], acc[3][j], b2[co0 + j],
                                     &arg);
      a2[((wy + 2) * S2P + wx + 2) * F + co0 + j] = v;
      pool2[b * NF + win * F + co0 + j] = v;
    }
  }
  __syncthreads();
  // conv3 + relu: a wave per channel pair, a lane per position
  for (int pos = lane; pos < N2; pos += 64) {
    const int y = pos / S2, xx = pos % S2;
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const float* w = w3 + (ky * 5 + kx) * F * F + co0;
        float in[F];
        load8(a2 + ((y + ky) * S2P + xx + kx) * F, in);
#pragma unroll
        for (int ci = 0; ci < F; ++ci) {
          acc0 = fmaf(in[ci], w[ci * F], acc0);
          acc1 = fmaf(in[ci], w[ci * F + 1], acc1);
        }
      }
    }
    feat[b * NF + pos * F + co0] = relu(acc0 + b3[co0]);
    feat[b * NF + pos * F + co0 + 1] = relu(acc1 + b3[co0 + 1]);
  }
}

// Backward of images [g ipw, min(B, (g+1) ipw)) -> partial sums part[g][PART].
// LDS regions along the phases of one image:
//   r1 (29 29 F floats): zero-bordered pool1 -> zero-bordered dL/dconv2 ->
//                        conv1's window gradients g1 [625, F] + argmax bytes
//   r3 (3200 floats):    zero-bordered pool2 + dL/dconv3 [144, F] -> the
//                        zero-bordered canvas
//   r4 (1440 floats):    conv2's window gradients g2 [144, F] + argmax bytes ->
//                        the chunk sums of conv1's weight / bias gradient
__global__ __launch_bounds__(NT) void cnn_enc_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ pool1, const float* __restrict__ pool2,
    const float* __restrict__ feat, const float* __restrict__ dF, int B, int ipw,
    float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float r1[S1P * S1P * F];           // 26,912 B
  __shared__ __attribute__((aligned(16))) float r3[S2P * S2P * F + NF];      // 12,800 B
  __shared__ __attribute__((aligned(16))) float r4[NF + NF / 4];             //  5,760 B
  static_assert(S2P * S2P * F + NF >= XP * XP, "the canvas fits r3");
  static_assert(N1 * F + N1 * F / 4 <= S1P * S1P * F, "g1 and its argmax bytes fit r1");
  static_assert(CH1 * (KW1 + F) <= NF + NF / 4, "conv1's chunk sums fit r4");
  static_assert(CH1 * CH1_WIN >= N1 && CH1 * 5 * F <= NT, "conv1 weight-gradient chunks");
  float* const a2 = r3;                    // zero-bordered pool2
  float* const d3 = r3 + S2P * S2P * F;    // dL/d(conv3 before relu) [144, F]
  float* const g2 = r4;                    // dL/d(conv2 before relu) at each window's argmax
  unsigned char* const arg2 = reinterpret_cast<unsigned char*>(r4 + NF);
  float* const g1 = r1;
  unsigned char* const arg1 = reinterpret_cast<unsigned char*>(r1 + N1 * F);
  float* const sum1 = r4;                  // [CH1][KW1] then [CH1][F]
  const int t = threadIdx.x, lane = t & 63;
  const int co0 = 2 * __builtin_amdgcn_readfirstlane(t >> 6);
  const int co = t & 7;                    // the channel of this thread's kernel elements
  // this thread's conv2 / conv3 kernel elements t + 256 j = (k_j, co), k = (ky 5 + kx) F + ci
  int off2[WJ], off3[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int k = (t >> 3) + 32 * j, tap = (k >> 3) % 25, ci = k & 7;  // (% 25: j = 6 of t >= 64 is unused)
    off2[j] = ((tap / 5) * S1P + tap % 5) * F + ci;
    off3[j] = ((tap / 5) * S2P + tap % 5) * F + ci;
  }
  const int nj = t < KW2 - (WJ - 1) * NT ? WJ : WJ - 1;
  float aw3[WJ], aw2[WJ], aw1 = 0.0f, ab1 = 0.0f, ab2 = 0.0f, ab3 = 0.0f;
#pragma unroll
  for (int j = 0; j < WJ; ++j) aw3[j] = aw2[j] = 0.0f;

  const int img0 = blockIdx.x * ipw, img1 = min(B, img0 + ipw);
  for (int img = img0; img < img1; ++img) {
    const size_t b = img;
    __syncthreads();  // the previous image's readers of r1, r3, r4 are done
    load_plane(r1, pool1 + b * (N1 * F), S1, t);
    load_plane(a2, pool2 + b * NF, S2, t);
    for (int i = t; i < NF; i += NT) d3[i] = feat[b * NF + i] > 0.0f ? dF[b * NF + i] : 0.0f;
    __syncthreads();
    // ---- conv3: weight gradient (all positions, in order), bias gradient
    for (int y = 0; y < S2; ++y)
      for (int xx = 0; xx < S2; ++xx) {
        const float g = d3[(y * S2 + xx) * F + co];
        const float* a = a2 + (y * S2P + xx) * F;
#pragma unroll
        for (int j = 0; j < WJ; ++j)
          if (j < nj) aw3[j] = fmaf(a[off3[j]], g, aw3[j]);
      }
    if (t < F)
      for (int pos = 0; pos < N2; ++pos) ab3 += d3[pos * F + t];
    // ---- dL/dpool2 (kept in registers), then conv2's windows recomputed:
    // a wave per channel pair, a lane per pool2 position = conv2 window
    for (int win = lane; win < N2; win += 64) {
      const int wy = win / S2, wx = win % S2;
      float dp0 = 0.0f, dp1 = 0.0f;
      for (int ky = 0; ky < 5; ++ky) {
        const int yy = wy + 2 - ky;
        if (yy < 0 || yy >= S2) continue;
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
          const int xq = wx + 2 - kx;
          if (xq < 0 || xq >= S2) continue;
          float d[F];
          load8(d3 + (yy * S2 + xq) * F, d);
          const float* w = w3 + ((ky * 5 + kx) * F + co0) * F;  // [ci = co0 (+1)][co]
#pragma unroll
          for (int c = 0; c < F; ++c) {
            dp0 = fmaf(d[c], w[c], dp0);
            dp1 = fmaf(d[c], w[F + c], dp1);
          }
        }
      }
      float acc[4][2];
      conv2_window(r1, w2, wy, wx, co0, acc);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int arg;
        const float v = pool_first_max(acc[0][j], acc[1][j], acc[2][j], acc[3][j], b2[co0 + j],
                                       &arg);
        g2[win * F + co0 + j] = v > 0.0f ? (j ? dp1 : dp0) : 0.0f;
        arg2[win * F + co0 + j] = (unsigned char)arg;
      }
    }
    __syncthreads();
    // ---- conv2: weight gradient from each window's argmax tap, bias gradient;
    // the canvas into r3 (pool2 and d3 are dead)
    load_x(r3, x + b * (C * C), t);
    for (int win = 0; win < N2; ++win) {
      const float g = g2[win * F + co];
      const int a = arg2[win * F + co];
      const float* p = r1 + ((2 * (win / S2) + (a >> 1)) * S1P + 2 * (win % S2) + (a & 1)) * F;
#pragma unroll
      for (int j = 0; j < WJ; ++j)
        if (j < nj) aw2[j] = fmaf(p[off2[j]], g, aw2[j]);
    }
    if (t < F)
      for (int win = 0; win < N2; ++win) ab2 += g2[win * F + t];
    __syncthreads();
    // ---- r1 := zero-bordered dL/d(conv2 before relu) (row / column 24 zero)
    for (int i = t; i < S1P * S1P * F; i += NT) r1[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < NF; i += NT) {
      const int win = i >> 3, a = arg2[i];
      r1[((2 * (win / S2) + (a >> 1) + 2) * S1P + 2 * (win % S2) + (a & 1) + 2) * F + (i & 7)] =
          g2[i];
    }
    __syncthreads();
    // ---- dL/dpool1 in registers: a thread per position, all channels
    float dp[3][F];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int ci = 0; ci < F; ++ci) dp[r][ci] = 0.0f;
      const int pos = t + r * NT;
      if (pos < N1) {
        const int y = pos / S1, xx = pos % S1;
        for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 5; ++kx) {
            // conv2 position (y + 2 - ky, x + 2 - kx), + 2 for the border
            float d[F];
            load8(r1 + ((y + 4 - ky) * S1P + xx + 4 - kx) * F, d);
            const float* w = w2 + (ky * 5 + kx) * F * F;
#pragma unroll
            for (int ci = 0; ci < F; ++ci)
#pragma unroll
              for (int c = 0; c < F; ++c) dp[r][ci] = fmaf(d[c], w[ci * F + c], dp[r][ci]);
          }
        }
      }
    }
    __syncthreads();  // dL/dconv2 is read: r1 := g1, arg1
    // ---- conv1's windows recomputed
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int win = t + r * NT;
      if (win < N1) {
        float acc[4][F];
        conv1_window(r3, w1, win / S1, win % S1, acc);
#pragma unroll
        for (int c = 0; c < F; ++c) {
          int arg;
          const float v = pool_first_max(acc[0][c], acc[1][c], acc[2][c], acc[3][c], b1[c], &arg);
          g1[win * F + c] = v > 0.0f ? dp[r][c] : 0.0f;
          arg1[win * F + c] = (unsigned char)arg;
        }
      }
    }
    __syncthreads();
    // ---- conv1: weight / bias gradient in CH1 chunks of windows, thread
    // (chunk, ky, co) with the five kx in registers; the chunks added in order
    if (t < CH1 * 5 * F) {
      const int chunk = t / (5 * F), ky = (t % (5 * F)) >> 3;
      float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, sb = 0.0f;
      const int wend = min(N1, (chunk + 1) * CH1_WIN);
      for (int win = chunk * CH1_WIN; win < wend; ++win) {
        const float g = g1[win * F + co];
        const int a = arg1[win * F + co];
        const float* p = r3 + (2 * (win / S1) + (a >> 1) + ky) * XP + 2 * (win % S1) + (a & 1);
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) s[kx] = fmaf(p[kx], g, s[kx]);
        sb += g;
      }
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) sum1[chunk * KW1 + (ky * 5 + kx) * F + co] = s[kx];
      if (ky == 0) sum1[CH1 * KW1 + chunk * F + co] = sb;
    }
    __syncthreads();
    if (t < KW1)
      for (int c = 0; c < CH1; ++c) aw1 += sum1[c * KW1 + t];
    if (t < F)
      for (int c = 0; c < CH1; ++c) ab1 += sum1[CH1 * KW1 + c * F + t];
  }
  float* out = part + (size_t)blockIdx.x * PART;
  if (t < KW1) out[OFF_W1 + t] = aw1;
  if (t < F) out[OFF_B1 + t] = ab1, out[OFF_B2 + t] = ab2, out[OFF_B3 + t] = ab3;
#pragma unroll
  for (int j = 0; j < WJ; ++j)
    if (j < nj) out[OFF_W2 + t + j * NT] = aw2[j], out[OFF_W3 + t + j * NT] = aw3[j];
}

struct GradPtrs {
  float* p[6];  // w1, b1, w2, b2, w3, b3
};

// grad[i] = sum_g part[g][i]: 64 elements per workgroup, wave s sums the
// workgroups of slice s in index order, the four slices are added in order.
__global__ __launch_bounds__(NT) void cnn_enc_reduce_kernel(const float* __restrict__ part,
                                                           int nwg, GradPtrs out) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int per = (nwg + 3) / 4;
  float acc = 0.0f;
  if (i < PART)
    for (int g = s * per; g < min(nwg, (s + 1) * per); ++g) acc += part[(size_t)g * PART + i];
  red[s][lane] = acc;
  __syncthreads();
  if (s == 0 && i < PART) {
    const float v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (i < OFF_B1) out.p[0][i - OFF_W1] = v;
    else if (i < OFF_W2) out.p[1][i - OFF_B1] = v;
    else if (i < OFF_B2) out.p[2][i - OFF_W2] = v;
    else if (i < OFF_W3) out.p[3][i - OFF_B2] = v;
    else if (i < OFF_B3) out.p[4][i - OFF_W3] = v;
    else out.p[5][i - OFF_B3] = v;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mog_cnn_enc_images_per_wg(int B) {
  const int n = B / 512;
  return n < 1 ? 1 : n > MAX_IPW ? MAX_IPW : n;
}

extern "C" long mog_cnn_enc_partial_elems(int B, int images_per_wg) {
  if (B <= 0 || images_per_wg < 1 || images_per_wg > MAX_IPW) return 0;
  return (long)((B + images_per_wg - 1) / images_per_wg) * PART;
}

extern "C" int mog_cnn_enc_forward(const float* x, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const float* w3,
                                   const float* b3, int B, int filters, float* pool1,
                                   float* pool2, float* feat, void* stream) {
  MOG_CHECK_ARG(x && w1 && b1 && w2 && b2 && w3 && b3 && pool1 && pool2 && feat);
  MOG_CHECK_ARG(B >= 0 && filters == F);
  MOG_CHECK_ARG(aligned16(pool1) && aligned16(pool2));
  if (B == 0) return 0;
  hipLaunchKernelGGL(cnn_enc_forward_kernel, dim3(B), dim3(NT), 0, mog_stream(stream), x, w1, b1,
                     w2, b2, w3, b3, pool1, pool2, feat);
  MOG_LAUNCH_RET();
}

extern "C" int mog_cnn_enc_backward(const float* x, const float* w1, const float* b1,
                                    const float* w2, const float* b2, const float* w3,
                                    const float* pool1, const float* pool2, const float* feat,
                                    const float* dF, int B, int filters, int images_per_wg,
                                    float* part, long part_elems, float* gw1, float* gb1,
                                    float* gw2, float* gb2, float* gw3, float* gb3,
                                    void* stream) {
  MOG_CHECK_ARG(x && w1 && b1 && w2 && b2 && w3 && pool1 && pool2 && feat && dF && part);
  MOG_CHECK_ARG(gw1 && gb1 && gw2 && gb2 && gw3 && gb3);
  MOG_CHECK_ARG(B >= 0 && filters == F && images_per_wg >= 1 && images_per_wg <= MAX_IPW);
  MOG_CHECK_ARG(part_elems >= mog_cnn_enc_partial_elems(B, images_per_wg));
  MOG_CHECK_ARG(aligned16(pool1) && aligned16(pool2));
  if (B == 0) return 0;
  const int nwg = (B + images_per_wg - 1) / images_per_wg;
  hipStream_t s = mog_stream(stream);
  hipLaunchKernelGGL(cnn_enc_backward_kernel, dim3(nwg), dim3(NT), 0, s, x, w1, b1, w2, b2, w3,
                     pool1, pool2, feat, dF, B, images_per_wg, part);
  MOG_TRY((int)hipGetLastError());
  GradPtrs out = {{gw1, gb1, gw2, gb2, gw3, gb3}};
  hipLaunchKernelGGL(cnn_enc_reduce_kernel, dim3(mog_cdiv(PART, 64)), dim3(NT), 0, s, part, nwg,
                     out);
  MOG_LAUNCH_RET();
}
