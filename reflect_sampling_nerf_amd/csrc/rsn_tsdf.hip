// Depth-map fusion into a truncated signed distance volume (include/rsn.h, "TSDF fusion").
//
// One lane per grid vertex, x fastest: the lanes of a wave hold neighbouring vertices of one grid row, so the loads and stores of
// T and W are contiguous, and their projections into a view are neighbouring pixels, so the depth gather of a wave touches a few
// cache lines of a few image rows.  A lane reads its T and W once, walks the call's views in ascending order with both words in
// registers and stores them once: 16 bytes of volume traffic per vertex and call, whatever the number of views.  The poses are
// read at a view index that is the same in every lane (scalar loads); the intrinsics are kernel arguments.  No atomics, no LDS:
// every output word has one owner, so the result is deterministic.
//
// Every arithmetic step is one correctly rounded fp32 operation in the order the header states: the library is built with
// -ffp-contract=off (no fused multiply-add), and hipcc's `/` and sqrtf on fp32 are the correctly rounded forms (its default
// -fhip-fp32-correctly-rounded-divide-sqrt; the __fdiv_rn / __fsqrt_rn spellings map to the same or, for the root, to the
// faster 1-ulp instruction, so they are not used).  tests/test_tsdf_gpu.py holds the kernel to the bits of a numpy restatement.
#include "rsn_common.h"

#include <math.h>

#define RSN_TSDF_BLOCK 256
#define RSN_TSDF_MAX_BLOCKS 2048            // the rest of a large grid is walked with a grid stride
#define RSN_TSDF_MAX_POINTS (1 << 27)       // the limit of the mesh calls, whose volumes these are

struct TsdfFrame {
  float o[3], s[3];
};

struct TsdfCamera {
  int height, width;
  float fx, fy, cx, cy;
};

__global__ __launch_bounds__(RSN_TSDF_BLOCK) void rsn_tsdf_integrate_kernel(int nx, int ny, int n, TsdfFrame fr, int n_views,
                                                                            const float* __restrict__ c2w, TsdfCamera cam,
                                                                            const float* __restrict__ depth, float trunc,
                                                                            float near, float* __restrict__ tsdf,
                                                                            float* __restrict__ weight) {
  const int nxy = nx * ny;
  // the sides as floats; past 2^24 the conversion rounds, and u < fw still implies floor(u) < width: fw is the float nearest to
  // width, so the next float below it lies below width
  const float fw = (float)cam.width, fh = (float)cam.height;
  const int64_t hw = (int64_t)cam.height * cam.width;
  for (int64_t p64 = (int64_t)blockIdx.x * RSN_TSDF_BLOCK + threadIdx.x; p64 < n; p64 += (int64_t)gridDim.x * RSN_TSDF_BLOCK) {
    const int p = (int)p64;
    const int k = p / nxy, rem = p - k * nxy, j = rem / nx, i = rem - j * nx;
    const float pos[3] = {fr.o[0] + fr.s[0] * (float)i, fr.o[1] + fr.s[1] * (float)j, fr.o[2] + fr.s[2] * (float)k};
    float T = tsdf[p], W = weight[p];
    bool touched = false;
    for (int view = 0; view < n_views; ++view) {
      const float* m = c2w + (size_t)view * 12;  // [3,4] row-major: m[4 a + c]
      const float q0 = pos[0] - m[3], q1 = pos[1] - m[7], q2 = pos[2] - m[11];
      const float cam0 = (m[0] * q0 + m[4] * q1) + m[8] * q2;
      const float cam1 = (m[1] * q0 + m[5] * q1) + m[9] * q2;
      const float cam2 = (m[2] * q0 + m[6] * q1) + m[10] * q2;
      const float z = -cam2;
      if (!(z > 0.0f)) continue;
      const float u = (cam.fx * cam0) / z + cam.cx;
      const float v = cam.cy - (cam.fy * cam1) / z;
      if (!(u >= 0.0f && u < fw && v >= 0.0f && v < fh)) continue;  // on the floats: a NaN skips
      const float r = sqrtf((q0 * q0 + q1 * q1) + q2 * q2);
      if (r < near) continue;
      const int x = (int)floorf(u), y = (int)floorf(v);  // 0 <= x < width, 0 <= y < height by the test above
      const float D = depth[(int64_t)view * hw + (int64_t)y * cam.width + x];
      if (!isfinite(D)) continue;
      const float s = D - r;
      if (s < -trunc) continue;  // hidden behind the surface this view saw
      const float d = fminf(1.0f, s / trunc);
      const float Wn = W + 1.0f;
      T = (T * W + d) / Wn;
      W = Wn;
      touched = true;
    }
    if (touched) {
      tsdf[p] = T;
      weight[p] = W;
    }
  }
}

extern "C" int rsn_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* origin3, const float* spacing3,
                                  int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx,
                                  float cy, const float* depth, float trunc, float near, float* tsdf, float* weight,
                                  void* stream) {
  RSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, RSN_ERR_INVALID_ARGUMENT,
              "tsdf grid %d x %d x %d: every dimension must be at least 2", nx, ny, nz);
  const int64_t nxy = (int64_t)nx * ny;
  RSN_REQUIRE(nxy <= RSN_TSDF_MAX_POINTS && nxy * nz <= RSN_TSDF_MAX_POINTS, RSN_ERR_UNSUPPORTED,
              "tsdf grid %d x %d x %d: more than 2^27 points (512^3)", nx, ny, nz);
  RSN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= INT32_MAX, RSN_ERR_INVALID_ARGUMENT,
              "tsdf: depth maps of %d x %d pixels: need height, width >= 1 and height * width <= 2^31 - 1", height, width);
  RSN_REQUIRE(n_views >= 0, RSN_ERR_INVALID_ARGUMENT, "tsdf: n_views=%d", n_views);
  RSN_REQUIRE(isfinite(trunc) && trunc > 0.0f, RSN_ERR_INVALID_ARGUMENT, "tsdf: trunc=%g: need a finite value above 0",
              (double)trunc);
  RSN_REQUIRE(isfinite(near), RSN_ERR_INVALID_ARGUMENT, "tsdf: near=%g: need a finite value", (double)near);
  RSN_REQUIRE(isfinite(fx) && isfinite(fy) && fx != 0.0f && fy != 0.0f, RSN_ERR_INVALID_ARGUMENT,
              "tsdf: fx=%g fy=%g: need finite, non-zero focal lengths", (double)fx, (double)fy);
  RSN_REQUIRE(n_views == 0 || (origin3 && spacing3 && c2w && depth && tsdf && weight), RSN_ERR_INVALID_ARGUMENT,
              "tsdf: a pointer is NULL");
  if (n_views == 0) return RSN_OK;
  TsdfFrame fr;
  for (int c = 0; c < 3; ++c) {
    fr.o[c] = origin3[c];
    fr.s[c] = spacing3[c];
  }
  const TsdfCamera cam{height, width, fx, fy, cx, cy};
  const int n = (int)(nxy * nz);
  const int64_t want = ((int64_t)n + RSN_TSDF_BLOCK - 1) / RSN_TSDF_BLOCK;
  const dim3 grid((unsigned)(want < RSN_TSDF_MAX_BLOCKS ? want : RSN_TSDF_MAX_BLOCKS)), block(RSN_TSDF_BLOCK);
  hipLaunchKernelGGL(rsn_tsdf_integrate_kernel, grid, block, 0, (hipStream_t)stream, nx, ny, n, fr, n_views, c2w, cam, depth, trunc,
                     near, tsdf, weight);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
