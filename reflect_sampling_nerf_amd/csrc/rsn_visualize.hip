// Per-pixel floats -> 8-bit RGB tiles of a panel (include/rsn.h, "visualisation").
//
// One lane per pixel: it reads its 1 or 3 floats (and its alpha) and stores its three bytes one by one -- a pixel's bytes start
// at an odd address two times out of three, and the neighbours to the left and right of a tile belong to other calls, so no lane
// ever writes outside the three bytes it owns (the compiler pairs two of them into one 2-byte store, which global memory takes
// at any address).  Every arithmetic step is one fp32 operation in the order the header states (the file is built with
// -ffp-contract=off like the rest of the library).  The launch is a few microseconds beside the field evaluation of a frame;
// it is not tuned.
#include "rsn_common.h"

#include <math.h>

#define RSN_VIS_BLOCK 256
#define RSN_VIS_MAX_BLOCKS 2048  // the rest of a large image is walked with a grid stride

// 0 for NaN, v <= 0 (so -0.0 and -inf), 1 for v > 1, else v
__device__ __forceinline__ float vis_sat(float v) { return v > 0.0f ? (v > 1.0f ? 1.0f : v) : 0.0f; }

// v in [0, 1] laid over white with coverage a, as a byte
__device__ __forceinline__ uint8_t vis_byte(float v, float a, float na) {
  const float o = v * a + na;
  return (uint8_t)(int)(o * 255.0f + 0.5f);
}

template <int KIND>
__global__ __launch_bounds__(RSN_VIS_BLOCK) void rsn_visualize_kernel(int n, int width, const float* __restrict__ x,
                                                                      const float* __restrict__ alpha, float lo, float hi,
                                                                      const float* __restrict__ lut, uint8_t* __restrict__ out,
                                                                      int pitch, int x0) {
  for (int64_t p64 = (int64_t)blockIdx.x * RSN_VIS_BLOCK + threadIdx.x; p64 < n; p64 += (int64_t)gridDim.x * RSN_VIS_BLOCK) {
    const int p = (int)p64;
    const int y = p / width, col = p - y * width;
    const float a = alpha ? vis_sat(alpha[p]) : 1.0f;
    const float na = 1.0f - a;
    float c[3];
    if (KIND == RSN_VIS_RGB || KIND == RSN_VIS_UNIT) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float v = x[(size_t)p * 3 + k];
        c[k] = vis_sat(KIND == RSN_VIS_UNIT ? v * 0.5f + 0.5f : v);
      }
    } else {
      const float t = vis_sat((x[p] - lo) / (hi - lo));
      if (KIND == RSN_VIS_LUT) {
        const int k = (int)(t * 255.0f);  // t in [0, 1]: k in [0, 255]
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = lut[k * 3 + ch];
      } else {
        c[0] = c[1] = c[2] = t;
      }
    }
    uint8_t* o = out + ((size_t)y * pitch + x0 + col) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = vis_byte(c[k], a, na);
  }
}

extern "C" int rsn_visualize(int32_t height, int32_t width, int32_t kind, const float* x, const float* alpha, float lo,
                             float hi, const float* lut, uint8_t* out, int32_t pitch, int32_t x0, void* stream) {
  RSN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= INT32_MAX, RSN_ERR_INVALID_ARGUMENT,
              "visualize: %d x %d pixels: need height, width >= 1 and height * width <= 2^31 - 1", height, width);
  RSN_REQUIRE(x0 >= 0 && (int64_t)x0 + width <= pitch, RSN_ERR_INVALID_ARGUMENT,
              "visualize: tile [%d, %d + %d) does not lie in a row of %d pixels", x0, x0, width, pitch);
  RSN_REQUIRE(kind == RSN_VIS_RGB || kind == RSN_VIS_UNIT || kind == RSN_VIS_GRAY || kind == RSN_VIS_LUT,
              RSN_ERR_INVALID_ARGUMENT, "visualize: unknown kind %d", kind);
  RSN_REQUIRE(x && out, RSN_ERR_INVALID_ARGUMENT, "visualize: x or out is NULL");
  RSN_REQUIRE(kind != RSN_VIS_LUT || lut, RSN_ERR_INVALID_ARGUMENT, "visualize: RSN_VIS_LUT needs a table, lut is NULL");
  if (kind == RSN_VIS_GRAY || kind == RSN_VIS_LUT)
    RSN_REQUIRE(isfinite(lo) && isfinite(hi) && hi > lo, RSN_ERR_INVALID_ARGUMENT,
                "visualize: range lo=%g hi=%g: need finite values with hi > lo", (double)lo, (double)hi);
  const int n = height * width;
  const int64_t want = ((int64_t)n + RSN_VIS_BLOCK - 1) / RSN_VIS_BLOCK;
  const dim3 grid((unsigned)(want < RSN_VIS_MAX_BLOCKS ? want : RSN_VIS_MAX_BLOCKS)), block(RSN_VIS_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case RSN_VIS_RGB:
      hipLaunchKernelGGL(rsn_visualize_kernel<RSN_VIS_RGB>, grid, block, 0, st, n, width, x, alpha, lo, hi, lut, out, pitch, x0);
      break;
    case RSN_VIS_UNIT:
      hipLaunchKernelGGL(rsn_visualize_kernel<RSN_VIS_UNIT>, grid, block, 0, st, n, width, x, alpha, lo, hi, lut, out, pitch, x0);
      break;
    case RSN_VIS_GRAY:
      hipLaunchKernelGGL(rsn_visualize_kernel<RSN_VIS_GRAY>, grid, block, 0, st, n, width, x, alpha, lo, hi, lut, out, pitch, x0);
      break;
    default:
      hipLaunchKernelGGL(rsn_visualize_kernel<RSN_VIS_LUT>, grid, block, 0, st, n, width, x, alpha, lo, hi, lut, out, pitch, x0);
      break;
  }
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
