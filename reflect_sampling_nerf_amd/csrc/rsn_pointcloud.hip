// Depth maps of posed pinhole cameras into one deduplicated, ordered point set (include/rsn.h, "point cloud").
//
// One lane per pixel of the call, g fastest along an image row: the lanes of a wave read neighbouring depths and accumulations
// (contiguous), and the four neighbour depths of the edge test come from the same or the adjacent rows' cache lines, re-read from
// global memory.  The pose is read at a view index that differs in at most a few lanes of a wave; the intrinsics and the grid's
// frame are kernel arguments.
//
//   mark    candidate rule, then owner[cell] = min(owner[cell], g): an integer atomicMin, the feature's only atomic.  The minimum
//           does not depend on the order, so owner is deterministic.
//   select  three launches, the compaction of rsn_occupancy_compact_samples: (1) the kept flag of every pixel (candidate rule,
//           then owner[cell] == g) into the workspace, with the kept and the candidate count of every tile of 256 pixels; (2) one
//           workgroup turns the kept counts into offsets and their total into *n_points, and sums the candidate counts into
//           *n_candidates -- the one serial step: 256 tiles per iteration; (3) every tile places its kept pixels by wave ballots
//           and writes g and the point, recomputed by the same device function.  No atomics: the rows come in ascending g.
// Workgroups loop over tiles, so the grid is bounded whatever the number of pixels.
//
// Every arithmetic step of the rule is one correctly rounded fp32 operation in the header's order, spelled with __fmul_rn /
// __fadd_rn / __fsub_rn / __fdiv_rn so that none is contracted; the ray comes from camera_ray (rsn_camera.h), the function
// rsn_camera_rays_image runs.  tests/test_pointcloud_gpu.py holds the calls to the bits of a numpy restatement.
#include "rsn_camera.h"
#include "rsn_common.h"

#include <math.h>

#define RSN_PC_BLOCK 256
#define RSN_PC_MAX_BLOCKS 1024          // four workgroups per CU; past 262,144 pixels a workgroup walks several tiles
#define RSN_PC_MAX_CELLS (1 << 27)      // the limit of the mesh and TSDF calls
#define RSN_PC_NO_OWNER 0x7fffffff

struct PcArgs {
  int n_pixels;            // n_views * height * width of this call
  int height, width;
  int g0;                  // view0 * height * width: the global index of the call's first pixel
  Intrinsics k;
  const float* c2w;        // [n_views,3,4]
  const float* depth;      // [n_views, H*W]
  const float* acc;        // [n_views, H*W] or NULL
  float min_acc, edge;
  int nx, ny, nz;
  float fn[3];             // the cell counts as floats
  float org[3], spc[3];
};

__device__ __forceinline__ bool pc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN and the infinities

// the depth-edge test against one neighbour of the same view: true = the pixel is rejected
__device__ __forceinline__ bool pc_edge(float D, float Dn, float edge) {
  return pc_finite(Dn) && fabsf(__fsub_rn(D, Dn)) > __fmul_rn(edge, fminf(D, Dn));  // a NaN product compares false
}

// The candidate rule for pixel p of the call (0 <= p < a.n_pixels): -> is it a candidate; then pos = its point, *cell = its cell.
__device__ __forceinline__ bool pc_candidate(const PcArgs& a, int p, float* pos, int* cell) {
  const int hw = a.height * a.width;
  const int v = p / hw, pix = p - v * hw, y = pix / a.width, x = pix - y * a.width;
  const float* dv = a.depth + (size_t)v * hw;
  const float D = dv[pix];
  if (!(pc_finite(D) && D > 0.0f)) return false;
  if (a.acc && !(a.acc[(size_t)v * hw + pix] >= a.min_acc)) return false;  // a NaN fails
  if (y > 0 && pc_edge(D, dv[pix - a.width], a.edge)) return false;
  if (y + 1 < a.height && pc_edge(D, dv[pix + a.width], a.edge)) return false;
  if (x > 0 && pc_edge(D, dv[pix - 1], a.edge)) return false;
  if (x + 1 < a.width && pc_edge(D, dv[pix + 1], a.edge)) return false;
  float o[3], d[3], area;
  camera_ray(a.c2w + (size_t)v * 12, a.k, y, x, o, d, &area);
  int idx[3];
  bool inside = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pos[c] = __fadd_rn(o[c], __fmul_rn(D, d[c]));
    const float q = __fdiv_rn(__fsub_rn(pos[c], a.org[c]), a.spc[c]);
    inside = inside && q >= 0.0f && q < a.fn[c];  // on the floats: a NaN fails
    idx[c] = (int)floorf(q);                      // used only when inside: then 0 <= idx < n (fn is the float nearest to n)
  }
  if (!inside) return false;
  *cell = (idx[2] * a.ny + idx[1]) * a.nx + idx[0];
  return true;
}

__global__ __launch_bounds__(RSN_PC_BLOCK) void rsn_pointcloud_mark_kernel(const PcArgs a, int* __restrict__ owner) {
  for (int64_t p64 = (int64_t)blockIdx.x * RSN_PC_BLOCK + threadIdx.x; p64 < a.n_pixels; p64 += (int64_t)gridDim.x * RSN_PC_BLOCK) {
    const int p = (int)p64;
    float pos[3];
    int cell;
    if (pc_candidate(a, p, pos, &cell)) atomicMin(owner + cell, a.g0 + p);
  }
}

// kept[p] of every pixel, and the kept and the candidate count of every tile
__global__ __launch_bounds__(RSN_PC_BLOCK) void rsn_pointcloud_flag_kernel(const PcArgs a, int n_tiles, const int* __restrict__ owner,
                                                                           uint8_t* __restrict__ kept, int* __restrict__ tile_counts,
                                                                           int* __restrict__ cand_counts) {
  __shared__ int s_wave_tot[2][RSN_PC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // the bound is the same in every lane
    const int64_t p64 = (int64_t)tile * RSN_PC_BLOCK + tid;
    bool cand = false, keep = false;
    if (p64 < a.n_pixels) {
      const int p = (int)p64;
      float pos[3];
      int cell;
      cand = pc_candidate(a, p, pos, &cell);
      keep = cand && (!owner || owner[cell] == a.g0 + p);
      kept[p] = keep ? 1 : 0;
    }
    const unsigned long long bal_keep = __ballot(keep), bal_cand = __ballot(cand);
    if (lane == 0) {
      s_wave_tot[0][wid] = __builtin_popcountll(bal_keep);
      s_wave_tot[1][wid] = __builtin_popcountll(bal_cand);
    }
    __syncthreads();
    if (tid < 2) {
      int t = 0;
#pragma unroll
      for (int wv = 0; wv < RSN_PC_BLOCK / 64; ++wv) t += s_wave_tot[tid][wv];
      (tid == 0 ? tile_counts : cand_counts)[tile] = t;
    }
    __syncthreads();  // s_wave_tot is read before the next tile writes it
  }
}

// One workgroup: counts[t] -> the number of kept pixels in the tiles in front of t (in place), their total -> *n_points; the sum
// of cand_counts -> *n_candidates (when asked for).
__global__ __launch_bounds__(RSN_PC_BLOCK) void rsn_pointcloud_scan_kernel(int n_tiles, int* __restrict__ counts,
                                                                           const int* __restrict__ cand_counts, int* __restrict__ n_points,
                                                                           int* __restrict__ n_candidates) {
  __shared__ int s_wave_tot[RSN_PC_BLOCK / 64];
  __shared__ int s_cand[RSN_PC_BLOCK / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  int cands = 0;
  for (int base = 0; base < n_tiles; base += RSN_PC_BLOCK) {  // the bound is the same in every lane
    const int j = base + tid;
    const int v = j < n_tiles ? counts[j] : 0;
    cands += j < n_tiles ? cand_counts[j] : 0;
    int x = v;  // inclusive scan of the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_wave_tot[wid] = x;
    __syncthreads();
    int wave_off = 0, tot = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_PC_BLOCK / 64; ++wv) {
      const int t = s_wave_tot[wv];
      if (wv < wid) wave_off += t;
      tot += t;
    }
    const int carry = s_carry;
    if (j < n_tiles) counts[j] = carry + wave_off + x - v;
    __syncthreads();  // every lane has read s_carry and s_wave_tot
    if (tid == 0) s_carry = carry + tot;
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cands += __shfl_xor(cands, off, 64);  // integer sums: the order does not matter
  if (lane == 0) s_cand[wid] = cands;
  __syncthreads();
  if (tid == 0) {
    *n_points = s_carry;
    if (n_candidates) {
      int t = 0;
#pragma unroll
      for (int wv = 0; wv < RSN_PC_BLOCK / 64; ++wv) t += s_cand[wv];
      *n_candidates = t;
    }
  }
}

__global__ __launch_bounds__(RSN_PC_BLOCK) void rsn_pointcloud_emit_kernel(const PcArgs a, int n_tiles, const uint8_t* __restrict__ kept,
                                                                           const int* __restrict__ tile_offsets,
                                                                           int* __restrict__ pixel_index, float* __restrict__ positions) {
  __shared__ int s_wave_tot[RSN_PC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p64 = (int64_t)tile * RSN_PC_BLOCK + tid;
    const bool keep = p64 < a.n_pixels && kept[p64] != 0;
    const unsigned long long bal = __ballot(keep);
    const int in_wave = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
    __syncthreads();
    int wave_off = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_PC_BLOCK / 64; ++wv)
      if (wv < wid) wave_off += s_wave_tot[wv];
    if (keep) {
      const int p = (int)p64;
      const size_t row = (size_t)(tile_offsets[tile] + wave_off + in_wave);  // kept pixels with a smaller index: 0 .. p
      float pos[3];
      int cell;
      pc_candidate(a, p, pos, &cell);  // true, as in the flag pass: the same function on the same inputs
      pixel_index[row] = a.g0 + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) positions[row * 3 + c] = pos[c];  // consecutive kept lanes write consecutive rows
    }
    __syncthreads();  // s_wave_tot is read before the next tile writes it
  }
}

// ------------------------------------------------------------------------------------------------------------------- host side
static bool pc_shape_ok(int64_t n_views, int64_t height, int64_t width) {  // n_views * height * width <= INT32_MAX, without overflow
  if (n_views < 0 || height < 1 || width < 1) return false;
  const int64_t hw = height * width;  // below 2^62
  return n_views == 0 || (hw <= (int64_t)INT32_MAX && n_views * hw <= (int64_t)INT32_MAX);  // n_views < 2^32: below 2^63
}

static size_t pc_tiles(int64_t n_pixels) { return (size_t)((n_pixels + RSN_PC_BLOCK - 1) / RSN_PC_BLOCK); }

extern "C" size_t rsn_pointcloud_workspace_bytes(int32_t n_views, int32_t height, int32_t width) {
  if (!pc_shape_ok(n_views, height, width)) {
    rsn_set_error("pointcloud: n_views=%d height=%d width=%d: need n_views >= 0, height, width >= 1 and n_views*height*width <= 2^31 - 1",
                  n_views, height, width);
    return 0;
  }
  const int64_t n = (int64_t)n_views * height * width;
  // the kept and the candidate counts of the tiles (int32, first: aligned), then one byte per pixel rounded up to a word; never 0
  // for a valid shape
  return 2 * (pc_tiles(n) + 1) * sizeof(int32_t) + (size_t)((n + 3) / 4) * 4;
}

// Everything the two calls check alike, in one order; fills the kernels' arguments.
static int pc_prepare(const char* who, int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx,
                      float cy, const float* depth, const float* accumulation, int32_t view0, int32_t nx, int32_t ny, int32_t nz,
                      const float* origin3, const float* spacing3, float min_accumulation, float edge, PcArgs* a) {
  RSN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, RSN_ERR_INVALID_ARGUMENT, "%s: grid of %d x %d x %d cells: every dimension must be at least 1",
              who, nx, ny, nz);
  const int64_t nxy = (int64_t)nx * ny;
  RSN_REQUIRE(nxy <= RSN_PC_MAX_CELLS && nxy * nz <= RSN_PC_MAX_CELLS, RSN_ERR_UNSUPPORTED,
              "%s: grid of %d x %d x %d cells: more than 2^27 (512^3)", who, nx, ny, nz);
  RSN_REQUIRE(height >= 1 && width >= 1, RSN_ERR_INVALID_ARGUMENT, "%s: depth maps of %d x %d pixels: need height, width >= 1", who,
              height, width);
  RSN_REQUIRE(n_views >= 0 && view0 >= 0, RSN_ERR_INVALID_ARGUMENT, "%s: n_views=%d view0=%d: need both >= 0", who, n_views, view0);
  RSN_REQUIRE(pc_shape_ok((int64_t)view0 + n_views, height, width), RSN_ERR_INVALID_ARGUMENT,
              "%s: (view0 + n_views) * height * width = (%d + %d) * %d * %d: the global pixel index must stay <= 2^31 - 1", who, view0,
              n_views, height, width);
  RSN_REQUIRE(isfinite(fx) && isfinite(fy) && fx != 0.0f && fy != 0.0f, RSN_ERR_INVALID_ARGUMENT,
              "%s: fx=%g fy=%g: need finite, non-zero focal lengths", who, (double)fx, (double)fy);
  RSN_REQUIRE(!isnan(min_accumulation), RSN_ERR_INVALID_ARGUMENT, "%s: min_accumulation is NaN", who);
  RSN_REQUIRE(!isnan(edge) && edge >= 0.0f, RSN_ERR_INVALID_ARGUMENT, "%s: edge=%g: need a value >= 0 (+inf switches the test off)", who,
              (double)edge);
  RSN_REQUIRE(n_views == 0 || (origin3 && spacing3 && c2w && depth), RSN_ERR_INVALID_ARGUMENT,
              "%s: origin3, spacing3, c2w or depth is NULL", who);
  a->nx = nx; a->ny = ny; a->nz = nz;
  const int n3[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) {
    a->fn[c] = (float)n3[c];
    a->org[c] = origin3 ? origin3[c] : 0.0f;
    a->spc[c] = spacing3 ? spacing3[c] : 1.0f;
    RSN_REQUIRE(isfinite(a->org[c]) && isfinite(a->spc[c]) && a->spc[c] > 0.0f, RSN_ERR_INVALID_ARGUMENT,
                "%s: axis %d: origin %g spacing %g: need finite values and spacing > 0", who, c, (double)a->org[c], (double)a->spc[c]);
  }
  const int64_t hw = n_views ? (int64_t)height * width : 0;  // a call without views launches nothing
  a->n_pixels = (int)(n_views * hw);
  a->height = height; a->width = width;
  a->g0 = (int)(view0 * hw);
  a->k = Intrinsics{fx, fy, cx, cy};
  a->c2w = c2w; a->depth = depth; a->acc = accumulation;
  a->min_acc = min_accumulation; a->edge = edge;
  return RSN_OK;
}

static unsigned pc_blocks(size_t tiles) { return (unsigned)(tiles < RSN_PC_MAX_BLOCKS ? tiles : RSN_PC_MAX_BLOCKS); }

extern "C" int rsn_pointcloud_mark(int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx,
                                   float cy, const float* depth, const float* accumulation, int32_t view0, int32_t nx, int32_t ny,
                                   int32_t nz, const float* origin3, const float* spacing3, float min_accumulation, float edge,
                                   int32_t* owner, void* stream) {
  PcArgs a;
  RSN_TRY(pc_prepare("pointcloud_mark", n_views, c2w, height, width, fx, fy, cx, cy, depth, accumulation, view0, nx, ny, nz, origin3,
                     spacing3, min_accumulation, edge, &a));
  if (n_views == 0 || !owner) return RSN_OK;  // without owner there is nothing to record
  hipLaunchKernelGGL(rsn_pointcloud_mark_kernel, dim3(pc_blocks(pc_tiles(a.n_pixels))), dim3(RSN_PC_BLOCK), 0, (hipStream_t)stream, a,
                     owner);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_pointcloud_select(int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx,
                                     float cy, const float* depth, const float* accumulation, int32_t view0, int32_t nx, int32_t ny,
                                     int32_t nz, const float* origin3, const float* spacing3, float min_accumulation, float edge,
                                     const int32_t* owner, void* workspace, size_t workspace_bytes, int32_t* n_points,
                                     int32_t* n_candidates, int32_t* pixel_index, float* positions, void* stream) {
  PcArgs a;
  RSN_TRY(pc_prepare("pointcloud_select", n_views, c2w, height, width, fx, fy, cx, cy, depth, accumulation, view0, nx, ny, nz, origin3,
                     spacing3, min_accumulation, edge, &a));
  RSN_REQUIRE(n_points, RSN_ERR_INVALID_ARGUMENT, "pointcloud_select: n_points is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (n_views == 0) {
    RSN_HIP(hipMemsetAsync(n_points, 0, sizeof(int32_t), st));
    if (n_candidates) RSN_HIP(hipMemsetAsync(n_candidates, 0, sizeof(int32_t), st));
    return RSN_OK;
  }
  RSN_REQUIRE(workspace && pixel_index && positions, RSN_ERR_INVALID_ARGUMENT,
              "pointcloud_select: workspace, pixel_index or positions is NULL");
  RSN_REQUIRE(((uintptr_t)workspace & 3u) == 0, RSN_ERR_INVALID_ARGUMENT, "pointcloud_select: workspace must be 4-byte aligned");
  const size_t need = rsn_pointcloud_workspace_bytes(n_views, height, width);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "pointcloud_select: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const size_t tiles = pc_tiles(a.n_pixels);
  int* counts = (int*)workspace;
  int* cand_counts = counts + tiles + 1;
  uint8_t* kept = (uint8_t*)(cand_counts + tiles + 1);
  const dim3 grid(pc_blocks(tiles)), block(RSN_PC_BLOCK);
  hipLaunchKernelGGL(rsn_pointcloud_flag_kernel, grid, block, 0, st, a, (int)tiles, owner, kept, counts, cand_counts);
  hipLaunchKernelGGL(rsn_pointcloud_scan_kernel, dim3(1), block, 0, st, (int)tiles, counts, cand_counts, n_points, n_candidates);
  hipLaunchKernelGGL(rsn_pointcloud_emit_kernel, grid, block, 0, st, a, (int)tiles, kept, counts, pixel_index, positions);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
