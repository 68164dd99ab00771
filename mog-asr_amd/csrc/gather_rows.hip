// Row gather of a device-resident dataset: the training batch of a shuffled
// pick list without a host gather or upload (records.DeviceFeed).
//   out[b, :] = src[idx[b], :]   (fp32 rows of `width` floats)
//   kout[b]   = ksrc[idx[b]]     (the int32 digit counts), same launch
// One workgroup per (row, 1024-float4 slice).  16-byte accesses when the width
// is a multiple of 4 floats and both bases are 16-byte aligned (2500 and 4096
// are), dwords otherwise.  An index outside [0, rows) copies nothing (the
// Python wrapper refuses it before any launch).
#include "mog_common.h"

namespace {

constexpr int NT = 256, VEC_PER_WG = 1024;

template <bool VEC>
__global__ __launch_bounds__(NT) void gather_rows_kernel(const float* __restrict__ src,
                                                         const int* __restrict__ ksrc,
                                                         const int* __restrict__ idx, int rows,
                                                         int width, float* __restrict__ out,
                                                         int* __restrict__ kout) {
  const int b = blockIdx.x;
  const int r = idx[b];
  if (r < 0 || r >= rows) return;
  if (blockIdx.y == 0 && threadIdx.x == 0 && ksrc != nullptr) kout[b] = ksrc[r];
  const float* s = src + (size_t)r * width;
  float* d = out + (size_t)b * width;
  if (VEC) {
    const int n4 = width >> 2;
    const floatx4* s4 = reinterpret_cast<const floatx4*>(s);
    floatx4* d4 = reinterpret_cast<floatx4*>(d);
    const int end = min(n4, (int)(blockIdx.y + 1) * VEC_PER_WG);
    for (int j = blockIdx.y * VEC_PER_WG + threadIdx.x; j < end; j += NT) d4[j] = s4[j];
  } else {
    const int end = min(width, (int)(blockIdx.y + 1) * VEC_PER_WG * 4);
    for (int j = blockIdx.y * VEC_PER_WG * 4 + threadIdx.x; j < end; j += NT) d[j] = s[j];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mog_gather_rows(const float* src, const int* ksrc, const int* idx, int rows,
                               int width, int B, float* out, int* kout, void* stream) {
  MOG_CHECK_ARG(rows >= 0 && width >= 1 && B >= 0 && (ksrc == nullptr) == (kout == nullptr));
  if (B == 0) return 0;
  MOG_CHECK_ARG(src && idx && out && rows >= 1 && width <= (1 << 28));
  const dim3 grid(B, mog_cdiv(width, VEC_PER_WG * 4)), block(NT);
  hipStream_t s = mog_stream(stream);
  if (width % 4 == 0 && aligned16(src) && aligned16(out))
    hipLaunchKernelGGL(gather_rows_kernel<true>, grid, block, 0, s, src, ksrc, idx, rows, width,
                       out, kout);
  else
    hipLaunchKernelGGL(gather_rows_kernel<false>, grid, block, 0, s, src, ksrc, idx, rows, width,
                       out, kout);
  MOG_LAUNCH_RET();
}
