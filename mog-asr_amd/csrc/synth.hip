// Training canvases made on the device (records.StreamFeed):
// image n of stream `seed` is a pure function of (seed, n), the placement of
// datasets.generate_multi_image restated over Philox words.
//
//   words(q)   = Philox4x32-10(key = seed, counter = {lo32(c), hi32(c), TAG, 0}),
//                c = n * 4096 + q;  an integer in [0, m) is (word * m) >> 32
//   quad 0     word 0 -> num = counts[pick]
//   block(r,j) the 51 quads from 1 + (r * GMAX + j) * 51 (restart r, object j):
//                quad 0 word 0 -> glyph id; attempt a reads quad 1 + a / 2,
//                words 2 (a % 2) and 2 (a % 2) + 1 -> x in [0, C - w], y in [0, C - h]
//   an attempt is accepted when no pixel has glyph > 0 and canvas > 0; an object
//   without a place in A attempts clears the canvas and starts restart r + 1;
//   after R restarts the image keeps what the last one had placed (status 1).
//
// One wave per image and no LDS canvas: lane L keeps row L's occupancy as a
// 64-bit mask (C <= 64) and, for the object being placed, the mask of glyph
// row L (L < 32).  Lanes 0..50 compute the block's 51 quads at once; an
// attempt is two word reads, one row-mask read (all three cross-lane), a
// shift, an AND and a vote.  Everything that steers a loop (num, glyph, x, y,
// the votes) is equal in all 64 lanes, so every cross-lane read and every vote
// runs with all lanes active; lanes without a canvas row vote false.  When the
// layout is final the canvas is written once: each pixel sums, in placement
// order, the glyph pixels that cover it (at most one is non-zero) and clips to
// [0, 1]; 16-byte stores when C * C is a multiple of 4 and the rows are
// 16-byte aligned.  No atomics, no barriers, no image reads another's data.
#include "mog_common.h"
#include "philox.h"

namespace {

constexpr int GMAX = 8, ATTEMPTS = 100, RESTARTS = 8, SIDE = 32;
constexpr int QUADS_PER_OBJECT = 1 + ATTEMPTS / 2;  // 51
constexpr int QUADS_PER_IMAGE = 4096;
constexpr uint32_t STREAM_TAG = 0x53594E54u;  // "SYNT": non-zero (the models' noise has 0)
constexpr int WAVES = 4;
static_assert(1 + RESTARTS * GMAX * QUADS_PER_OBJECT <= QUADS_PER_IMAGE, "quads per image");
static_assert(QUADS_PER_OBJECT <= MOG_WAVE && 2 * SIDE == MOG_WAVE, "one lane per quad");

__device__ __forceinline__ int below(uint32_t word, int m) {
  return (int)(((uint64_t)word * (uint32_t)m) >> 32);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// lane j < placed holds object j in (og, ox, oy, ow, oh)
struct Layout {
  int og, ox, oy, ow, oh;
};

__device__ __forceinline__ float pixel(const float* __restrict__ bank, const Layout& me,
                                       int placed, int row, int col) {
  float v = 0.0f;
#pragma unroll
  for (int j = 0; j < GMAX; ++j) {
    if (j < placed) {
      const int rr = row - __builtin_amdgcn_readlane(me.oy, j);
      const int cc = col - __builtin_amdgcn_readlane(me.ox, j);
      if ((unsigned)rr < (unsigned)__builtin_amdgcn_readlane(me.oh, j) &&
          (unsigned)cc < (unsigned)__builtin_amdgcn_readlane(me.ow, j))
        v += bank[(size_t)__builtin_amdgcn_readlane(me.og, j) * (SIDE * SIDE) + rr * SIDE + cc];
    }
  }
  return fminf(fmaxf(v, 0.0f), 1.0f);
}

template <bool VEC>
__global__ __launch_bounds__(WAVES* MOG_WAVE) void synth_kernel(
    const float* __restrict__ bank, const int* __restrict__ sizes, int G,
    const int* __restrict__ counts, int ncounts, int C, uint64_t seed, uint64_t first, int b,
    float* __restrict__ images, int* __restrict__ digits, int* __restrict__ objects,
    int* __restrict__ status) {
  const int lane = threadIdx.x & (MOG_WAVE - 1);
  const int img = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
  if (img >= b) return;  // the whole wave leaves: there is no barrier to miss
  const uint64_t base = (first + (uint64_t)img) * (uint64_t)QUADS_PER_IMAGE;

  uint32_t w[4];
  mog_philox_words(seed, base, STREAM_TAG, w);
  // (values the host wrapper has checked are clamped all the same: no device
  // value can push a loop or an address past its static bound)
  const int num = clampi(counts[below(w[0], ncounts)], 0, GMAX);

  uint64_t occ = 0;  // row `lane` of the canvas: bit c set where canvas > 0
  Layout me = {-1, -1, -1, -1, -1};
  int placed = 0, failed = 0;
  for (int r = 0; r < RESTARTS; ++r) {
    occ = 0;
    me = {-1, -1, -1, -1, -1};
    placed = 0;
    failed = 0;
    for (int j = 0; j < GMAX; ++j) {
      if (j >= num) break;
      // lanes 0..50: the block's quads (the lanes above repeat quad 50)
      const int q = 1 + (r * GMAX + j) * QUADS_PER_OBJECT + min(lane, QUADS_PER_OBJECT - 1);
      mog_philox_words(seed, base + (uint64_t)q, STREAM_TAG, w);
      const int g = below(__builtin_amdgcn_readfirstlane(w[0]), G);
      const int h = clampi(sizes[2 * g], 1, min(SIDE, C));
      const int gw = clampi(sizes[2 * g + 1], 1, min(SIDE, C));
      // glyph row masks: two rows of 32 pixels per vote, lane L keeps row L
      const float* gp = bank + (size_t)g * (SIDE * SIDE);
      uint32_t gm = 0;
#pragma unroll 4
      for (int i = 0; i < SIDE / 2; ++i) {
        const uint64_t two = __ballot(gp[i * MOG_WAVE + lane] > 0.0f);
        if ((lane >> 1) == i) gm = (uint32_t)(two >> ((lane & 1) * 32));
      }
      if (lane >= h) gm = 0;
      gm &= gw >= 32 ? 0xFFFFFFFFu : ((1u << gw) - 1u);

      int x = 0, y = 0, ok = 0;
      uint64_t mine = 0;
      for (int a = 0; a < ATTEMPTS; ++a) {
        const int src = 1 + (a >> 1);
        const uint32_t wx = (uint32_t)__shfl((int)((a & 1) ? w[2] : w[0]), src, MOG_WAVE);
        const uint32_t wy = (uint32_t)__shfl((int)((a & 1) ? w[3] : w[1]), src, MOG_WAVE);
        x = below(wx, C - gw + 1);
        y = below(wy, C - h + 1);
        // canvas row `lane` meets glyph row lane - y
        const int rel = lane - y;
        const uint32_t m = (uint32_t)__shfl((int)gm, rel & (MOG_WAVE - 1), MOG_WAVE);
        mine = (rel >= 0 && rel < h) ? ((uint64_t)m << x) : 0ull;
        if (!__any((mine & occ) != 0ull)) {
          ok = 1;
          break;
        }
      }
      if (!ok) {
        failed = 1;
        break;
      }
      occ |= mine;
      if (lane == j) me = {g, x, y, gw, h};
      ++placed;
    }
    if (!failed) break;
  }

  if (lane == 0) {
    digits[img] = placed;
    status[img] = failed;
  }
  if (lane < GMAX) {
    int* o = objects + ((size_t)img * GMAX + lane) * 5;
    o[0] = me.og;
    o[1] = me.ox;
    o[2] = me.oy;
    o[3] = me.ow;
    o[4] = me.oh;
  }

  const int npix = C * C;
  float* out = images + (size_t)img * npix;
  if (VEC) {
    floatx4* out4 = reinterpret_cast<floatx4*>(out);
    for (int i = lane; i < (npix >> 2); i += MOG_WAVE) {
      int row = (4 * i) / C, col = 4 * i - row * C;
      floatx4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = pixel(bank, me, placed, row, col);
        if (++col == C) {
          col = 0;
          ++row;
        }
      }
      out4[i] = v;
    }
  } else {
    for (int p = lane; p < npix; p += MOG_WAVE) {
      const int row = p / C;
      out[p] = pixel(bank, me, placed, row, p - row * C);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mog_synth_canvases(const float* bank, const int* sizes, int G, const int* counts,
                                  int ncounts, int C, unsigned long long seed,
                                  unsigned long long first, int b, float* images, int* digits,
                                  int* objects, int* status, void* stream) {
  MOG_CHECK_ARG(G >= 1 && G <= (1 << 20) && ncounts >= 1 && C >= SIDE && C <= MOG_WAVE && b >= 0);
  // n * 4096 + q stays below 2^64
  MOG_CHECK_ARG(first <= (1ull << 52) && (unsigned long long)b <= (1ull << 52) - first);
  if (b == 0) return 0;
  MOG_CHECK_ARG(bank && sizes && counts && images && digits && objects && status);
  const dim3 grid(mog_cdiv(b, WAVES)), block(WAVES * MOG_WAVE);
  hipStream_t s = mog_stream(stream);
  if ((C * C) % 4 == 0 && aligned16(images))
    hipLaunchKernelGGL(synth_kernel<true>, grid, block, 0, s, bank, sizes, G, counts, ncounts, C,
                       (uint64_t)seed, (uint64_t)first, b, images, digits, objects, status);
  else
    hipLaunchKernelGGL(synth_kernel<false>, grid, block, 0, s, bank, sizes, G, counts, ncounts, C,
                       (uint64_t)seed, (uint64_t)first, b, images, digits, objects, status);
  MOG_LAUNCH_RET();
}
