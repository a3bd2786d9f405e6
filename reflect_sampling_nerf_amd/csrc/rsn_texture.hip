// The sample point and footprint of every texel of a per-triangle texture atlas (include/rsn.h, "texture atlas").
//
// One lane per texel, the flat index row*N + col fastest along an image row: the lanes of a wave write neighbouring words of face and
// footprint and neighbouring 12-byte rows of point (contiguous per wave).  The P*P texels of a square read the same two triangles and
// six vertices, P of them side by side in a wave, so the reads of triangles and positions come from cache lines the neighbours
// share; the traffic that matters is the 20 bytes every texel writes.  A texel is owned by exactly one lane and every lane
// writes its texel's words unconditionally (the unused ones as -1 / 0): no atomics, nothing to order.
// Workgroups loop over tiles of 256 texels, so the grid is bounded whatever the size of the texture.
//
// Every arithmetic step is one correctly rounded fp32 operation in the header's order, spelled with __fmul_rn / __fadd_rn /
// __fsub_rn / __fdiv_rn so that none is contracted; the root is sqrtf, hipcc's correctly rounded form (__fsqrt_rn maps to the
// 1-ulp instruction).  tests/test_texture_gpu.py holds the call to the bits of a numpy restatement.
#include "rsn_common.h"

#include <math.h>

#define RSN_TEX_BLOCK 256
#define RSN_TEX_MAX_BLOCKS 2048      // eight workgroups per CU; past 524,288 texels a workgroup walks several tiles
#define RSN_TEX_MAX_SIZE 16384       // N*N <= 2^28 texels: the flat index and 3 * index fit an int32

struct TexArgs {
  int n_vertices, n_triangles;
  int P, Q, N;               // texels per square side, squares per row, N = Q*P
  int n_texels;              // N*N
  float fd;                  // (float)(P-3)
  const float* positions;    // [n_vertices,3]
  const int* triangles;      // [n_triangles,3]
};

__device__ __forceinline__ float tex_length(const float* p, const float* q) {
  const float dx = __fsub_rn(p[0], q[0]), dy = __fsub_rn(p[1], q[1]), dz = __fsub_rn(p[2], q[2]);
  return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

__global__ __launch_bounds__(RSN_TEX_BLOCK) void rsn_texture_points_kernel(const TexArgs a, int* __restrict__ face,
                                                                           float* __restrict__ point, float* __restrict__ footprint) {
  for (int64_t i64 = (int64_t)blockIdx.x * RSN_TEX_BLOCK + threadIdx.x; i64 < a.n_texels; i64 += (int64_t)gridDim.x * RSN_TEX_BLOCK) {
    const unsigned i = (unsigned)i64;                       // < 2^28
    const unsigned N = (unsigned)a.N, P = (unsigned)a.P;
    const unsigned row = i / N, col = i - row * N;
    const unsigned sx = col / P, ca = col - sx * P, sy = row / P, cb = row - sy * P;
    const bool upper = ca + cb >= P - 1;
    const bool live = upper ? (ca >= 2 && cb >= 2) : (ca + 3 <= P && cb + 3 <= P);
    const int64_t t = 2 * ((int64_t)sy * a.Q + sx) + (upper ? 1 : 0);
    int f = -1;
    float p[3] = {0.0f, 0.0f, 0.0f}, h = 0.0f;
    if (live && t < a.n_triangles) {
      const int* tri = a.triangles + (size_t)t * 3;
      const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
      if (i0 >= 0 && i0 < a.n_vertices && i1 >= 0 && i1 < a.n_vertices && i2 >= 0 && i2 < a.n_vertices) {
        const float* p0 = a.positions + (size_t)i0 * 3;
        const float* p1 = a.positions + (size_t)i1 * 3;
        const float* p2 = a.positions + (size_t)i2 * 3;
        const float u = __fdiv_rn((float)(upper ? P - 1 - ca : ca), a.fd);
        const float v = __fdiv_rn((float)(upper ? P - 1 - cb : cb), a.fd);
        const float w0 = __fsub_rn(__fsub_rn(1.0f, u), v);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          p[c] = __fadd_rn(__fadd_rn(__fmul_rn(w0, p0[c]), __fmul_rn(u, p1[c])), __fmul_rn(v, p2[c]));
        h = __fdiv_rn(fmaxf(tex_length(p1, p0), tex_length(p2, p0)), a.fd);
        f = (int)t;
      }
    }
    face[i] = f;
    footprint[i] = h;
#pragma unroll
    for (int c = 0; c < 3; ++c) point[(size_t)i * 3 + c] = p[c];  // consecutive lanes write consecutive rows
  }
}

// ------------------------------------------------------------------------------------------------------------------- host side
extern "C" int rsn_texture_points(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles,
                                  int32_t texels, int32_t squares_per_row, int32_t* face, float* point, float* footprint,
                                  void* stream) {
  RSN_REQUIRE(texels >= 4, RSN_ERR_INVALID_ARGUMENT, "texture_points: texels=%d: a square needs at least 4 x 4 texels", texels);
  RSN_REQUIRE(squares_per_row >= 1, RSN_ERR_INVALID_ARGUMENT, "texture_points: squares_per_row=%d: need at least 1", squares_per_row);
  RSN_REQUIRE(n_vertices >= 0 && n_triangles >= 0, RSN_ERR_INVALID_ARGUMENT, "texture_points: n_vertices=%d n_triangles=%d: need both >= 0",
              n_vertices, n_triangles);
  RSN_REQUIRE(2 * (int64_t)squares_per_row * squares_per_row >= n_triangles, RSN_ERR_INVALID_ARGUMENT,
              "texture_points: %d squares per row hold 2*%d^2 triangles, fewer than n_triangles=%d", squares_per_row, squares_per_row,
              n_triangles);
  RSN_REQUIRE(n_triangles == 0 || (triangles && face && point && footprint && (positions || n_vertices == 0)), RSN_ERR_INVALID_ARGUMENT,
              "texture_points: positions, triangles, face, point or footprint is NULL");
  const int64_t n = (int64_t)squares_per_row * texels;
  RSN_REQUIRE(n <= RSN_TEX_MAX_SIZE, RSN_ERR_UNSUPPORTED, "texture_points: a texture of %lld x %lld texels (%d squares of %d per row): more than %d",
              (long long)n, (long long)n, squares_per_row, texels, RSN_TEX_MAX_SIZE);
  if (n_triangles == 0) return RSN_OK;
  TexArgs a;
  a.n_vertices = n_vertices; a.n_triangles = n_triangles;
  a.P = texels; a.Q = squares_per_row; a.N = (int)n;
  a.n_texels = (int)(n * n);
  a.fd = (float)(texels - 3);
  a.positions = positions; a.triangles = triangles;
  const int64_t tiles = ((int64_t)a.n_texels + RSN_TEX_BLOCK - 1) / RSN_TEX_BLOCK;
  hipLaunchKernelGGL(rsn_texture_points_kernel, dim3((unsigned)(tiles < RSN_TEX_MAX_BLOCKS ? tiles : RSN_TEX_MAX_BLOCKS)),
                     dim3(RSN_TEX_BLOCK), 0, (hipStream_t)stream, a, face, point, footprint);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
