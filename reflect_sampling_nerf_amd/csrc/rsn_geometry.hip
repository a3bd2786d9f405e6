// Geometry metrics of an eval view against a ground-truth normal map (include/rsn.h, "geometry metrics").
//
//   rsn_normal_error   per-pixel angle between the composited predicted normal and the decoded ground truth, its alpha-weighted
//                      mean, the alpha error of the accumulation and the count of scored pixels, all on the device
//   rsn_depth_error    a view's rendered depth against its target distances: sum |d - D|, sum (d - D)^2 and the count over the pixels
//                      with a target (and a live mask byte), by the same launch shape and the same fixed-order sums
//
// One lane per pixel in a grid-stride loop of at most RSN_NORMAL_ERROR_MAX_GROUPS workgroups of 256 lanes.  A lane reads its 12
// bytes of prediction, 3 bytes of ground-truth normal, the alpha byte (whose pixel's other three bytes travel with it) and, when
// given, 4 bytes of accumulation, and writes, when wanted, 4 bytes of error map: 19 to 27 bytes of traffic a pixel, no reuse, no LDS
// beside the reduction.  Every fp32 step of the per-pixel recipe is one operation in
// the order the header states (the file is built with -ffp-contract=off like the rest of the library).
//
// Sums.  Each lane adds its pixels' terms in fp64 in ascending pixel order; the lanes of a wave are added by a butterfly, the four
// waves of a workgroup in order, and the workgroup stores one record of four doubles at workspace[4 * blockIdx.x].  A second launch
// of one workgroup adds the records the same way (lane i holds record i: there are at most 256) and writes out[0..3].  The order of
// every addition is fixed by (n_pixels, pixel index) alone: no atomics, the same bits from run to run.
#include "rsn_common.h"

#include <math.h>

#define RSN_NE_BLOCK 256
static_assert(RSN_NORMAL_ERROR_MAX_GROUPS <= RSN_NE_BLOCK, "the final sum gives every record one lane of one workgroup");

namespace {

struct NormalErrorArgs {
  int32_t n_pixels;
  const float* normals;
  const float* accumulation;
  const uint8_t* gt_normals;
  const uint8_t* gt_rgba;
  const float* rotation;
  float* error_map;
  double* partial;  // [gridDim.x][4]: S1, S2, S3, n
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the four sums of the workgroup's lanes, in lane 0 of the workgroup: butterfly within each wave, then the waves in order
__device__ __forceinline__ void group_sum(double (&v)[4], double (*red)[4]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

__global__ __launch_bounds__(RSN_NE_BLOCK) void rsn_normal_error_kernel(const NormalErrorArgs a) {
  __shared__ double red[RSN_NE_BLOCK / 64][4];
  float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if (a.rotation) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.rotation[k];
  }
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  const int stride = (int)gridDim.x * RSN_NE_BLOCK;  // <= 2^16
  for (int i = (int)blockIdx.x * RSN_NE_BLOCK + (int)threadIdx.x; i < a.n_pixels; i += stride) {  // n_pixels <= 2^24: no overflow
    const int alpha = a.gt_rgba[4 * (size_t)i + 3];
    int m = 0;
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = 2 * (int)a.gt_normals[3 * (size_t)i + c] - 255;
      m = max(m, abs(v));
      g[c] = (float)v;
    }
    if (a.rotation) {
      const float g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) g[r] = (R[3 * r] * g0 + R[3 * r + 1] * g1) + R[3 * r + 2] * g2;
    }
    const bool valid = alpha > 0 && m > 1;
    const float p0 = a.normals[3 * (size_t)i], p1 = a.normals[3 * (size_t)i + 1], p2 = a.normals[3 * (size_t)i + 2];
    const float c0 = p1 * g[2] - p2 * g[1], c1 = p2 * g[0] - p0 * g[2], c2 = p0 * g[1] - p1 * g[0];
    const float s = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    const float d = (p0 * g[0] + p1 * g[1]) + p2 * g[2];
    const float theta = (s == 0.0f && d == 0.0f) ? 1.57079632679489662f : atan2f(s, d);
    const float deg = theta * 57.2957795130823209f;
    if (a.error_map) a.error_map[i] = valid ? deg : 0.0f;
    if (valid) {
      sum[0] += (double)alpha * (double)deg;
      sum[1] += (double)alpha;
      sum[3] += 1.0;
    }
    if (a.accumulation) sum[2] += fabs((double)a.accumulation[i] - (double)alpha / 255.0);
  }
  group_sum(sum, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.partial[4 * (size_t)blockIdx.x + k] = sum[k];
  }
}

__global__ __launch_bounds__(RSN_NE_BLOCK) void rsn_normal_error_reduce_kernel(const double* partial, int n_partial, int n_pixels,
                                                                               int has_accumulation, float* out) {
  __shared__ double red[RSN_NE_BLOCK / 64][4];
  const int tid = threadIdx.x;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  if (tid < n_partial) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = partial[4 * (size_t)tid + k];
  }
  group_sum(sum, red);
  if (tid == 0) {
    out[0] = (float)(sum[0] / sum[1]);  // 0 / 0 = NaN: no valid pixel
    out[1] = (float)(sum[1] / 255.0);
    out[2] = has_accumulation ? (float)(sum[2] / (double)n_pixels) : 0.0f;
    out[3] = (float)sum[3];
  }
}

// rsn_depth_error: the first pass.  Record: (sum |d - D|, sum (d - D)^2, 0, count) over the pixels with D > 0 (and a live mask byte).
__global__ __launch_bounds__(RSN_NE_BLOCK) void rsn_depth_error_kernel(int n_pixels, const float* depth, const float* target,
                                                                       const uint8_t* mask, double* partial) {
  __shared__ double red[RSN_NE_BLOCK / 64][4];
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  const int stride = (int)gridDim.x * RSN_NE_BLOCK;
  for (int i = (int)blockIdx.x * RSN_NE_BLOCK + (int)threadIdx.x; i < n_pixels; i += stride) {
    const float D = target[i];
    if (D > 0.0f && (!mask || mask[i] != 0)) {
      const double e = (double)depth[i] - (double)D;
      sum[0] += fabs(e);
      sum[1] += e * e;
      sum[3] += 1.0;
    }
  }
  group_sum(sum, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) partial[4 * (size_t)blockIdx.x + k] = sum[k];
  }
}

__global__ __launch_bounds__(RSN_NE_BLOCK) void rsn_depth_error_reduce_kernel(const double* partial, int n_partial, float* out) {
  __shared__ double red[RSN_NE_BLOCK / 64][4];
  const int tid = threadIdx.x;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  if (tid < n_partial) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = partial[4 * (size_t)tid + k];
  }
  group_sum(sum, red);
  if (tid == 0) {
    out[0] = (float)sum[0];
    out[1] = (float)sum[1];
    out[2] = (float)sum[3];
  }
}

inline int normal_error_groups(int32_t n_pixels) {
  const int want = (n_pixels + RSN_NE_BLOCK - 1) / RSN_NE_BLOCK;
  return want < RSN_NORMAL_ERROR_MAX_GROUPS ? want : RSN_NORMAL_ERROR_MAX_GROUPS;
}

}  // namespace

extern "C" size_t rsn_normal_error_workspace_bytes(int32_t n_pixels) {
  if (n_pixels <= 0 || n_pixels > RSN_NORMAL_ERROR_MAX_PIXELS) return 0;
  return (size_t)normal_error_groups(n_pixels) * 4 * sizeof(double);
}

extern "C" int rsn_normal_error(int32_t n_pixels, const float* normals, const float* accumulation, const uint8_t* gt_normals,
                                const uint8_t* gt_rgba, const float* rotation, float* error_map, void* workspace,
                                size_t workspace_bytes, float* out, void* stream) {
  RSN_REQUIRE(n_pixels >= 1 && n_pixels <= RSN_NORMAL_ERROR_MAX_PIXELS, RSN_ERR_INVALID_ARGUMENT,
              "normal_error: n_pixels=%d: need 1 <= n_pixels <= 2^24 (the pixel count is returned as a float)", n_pixels);
  RSN_REQUIRE(normals && gt_normals && gt_rgba && workspace && out, RSN_ERR_INVALID_ARGUMENT,
              "normal_error: normals, gt_normals, gt_rgba, workspace or out is NULL");
  const size_t need = rsn_normal_error_workspace_bytes(n_pixels);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "normal_error: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  RSN_REQUIRE(((uintptr_t)workspace & 7) == 0, RSN_ERR_INVALID_ARGUMENT, "normal_error: workspace must be 8-byte aligned");
  const int groups = normal_error_groups(n_pixels);
  const NormalErrorArgs a{n_pixels, normals, accumulation, gt_normals, gt_rgba, rotation, error_map, (double*)workspace};
  hipLaunchKernelGGL(rsn_normal_error_kernel, dim3((unsigned)groups), dim3(RSN_NE_BLOCK), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(rsn_normal_error_reduce_kernel, dim3(1), dim3(RSN_NE_BLOCK), 0, (hipStream_t)stream,
                     (const double*)workspace, groups, (int)n_pixels, accumulation ? 1 : 0, out);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_depth_error(int32_t n_pixels, const float* depth, const float* target, const uint8_t* mask, void* workspace,
                               size_t workspace_bytes, float* out, void* stream) {
  RSN_REQUIRE(n_pixels >= 1 && n_pixels <= RSN_NORMAL_ERROR_MAX_PIXELS, RSN_ERR_INVALID_ARGUMENT,
              "depth_error: n_pixels=%d: need 1 <= n_pixels <= 2^24 (the pixel count is returned as a float)", n_pixels);
  RSN_REQUIRE(depth && target && workspace && out, RSN_ERR_INVALID_ARGUMENT, "depth_error: depth, target, workspace or out is NULL");
  const size_t need = rsn_normal_error_workspace_bytes(n_pixels);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "depth_error: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  RSN_REQUIRE(((uintptr_t)workspace & 7) == 0, RSN_ERR_INVALID_ARGUMENT, "depth_error: workspace must be 8-byte aligned");
  const int groups = normal_error_groups(n_pixels);
  hipLaunchKernelGGL(rsn_depth_error_kernel, dim3((unsigned)groups), dim3(RSN_NE_BLOCK), 0, (hipStream_t)stream, (int)n_pixels, depth,
                     target, mask, (double*)workspace);
  hipLaunchKernelGGL(rsn_depth_error_reduce_kernel, dim3(1), dim3(RSN_NE_BLOCK), 0, (hipStream_t)stream, (const double*)workspace,
                     groups, out);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
