// Empty-space skipping (include/rsn.h, "occupancy"): a bit per grid cell, the rays whose segment crosses no occupied cell, and
// the write-back of results computed on the compacted rays.
//
//   build   one lane per cell; a wavefront's 64 decisions are one ballot = two words of the bit array, stored by lanes 0 and 32.
//           Cells past the last one vote 0, which is what the unused high bits of the last word must hold.
//   cull    one lane per ray: the segment in grid coordinates (vertex (i, j, k) at (i, j, k)), clipped to the box, then a 3-D DDA
//           over the cells it crosses.  The arithmetic is fp64: one ray costs a few hundred operations, the launch is a fraction of
//           a millisecond beside the field kernels, and fp64 keeps the decision exact far inside the 1e-3-cell band the header
//           allows, for any box a scene is likely to have.  Every boundary crossing is recomputed from the cell index, never
//           accumulated.  The compaction is the two-pass one of rsn_reflect_setup: per-block counts, then every block sums the
//           counts in front of it (and all of them, for the culled rays' base) and places its rays by wave ballots.  No atomics.
//   scatter one lane per float of the compacted rows.
//   samples the same decision per SAMPLE of a level (rsn_occupancy_compact_samples): one lane per sub-segment [t_i, t_i+1] through
//           occ_ray_hits -- the DDA then spans one to three cells, and R*S lanes fill the machine -- plus the footprint rule; block
//           counts, one workgroup that turns them into offsets (and the total), then every block places its samples by wave
//           ballots and copies a live sample's ray and interval to its compact row.  rsn_scatter_level writes every member of a
//           level back in one launch, zeros in the rows of the skipped samples.  No atomics.
#include "rsn_common.h"

#include <math.h>

#define RSN_OCC_BLOCK 256
#define RSN_OCC_MAX_POINTS (1 << 27)

static bool occ_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz <= RSN_OCC_MAX_POINTS;
}

static int64_t occ_cells(int nx, int ny, int nz) { return (int64_t)(nx - 1) * (ny - 1) * (nz - 1); }

extern "C" size_t rsn_occupancy_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (!occ_dims_ok(nx, ny, nz)) {
    rsn_set_error("occupancy: grid %d x %d x %d: need every dimension >= 2 and nx*ny*nz <= 2^27", nx, ny, nz);
    return 0;
  }
  return (size_t)((occ_cells(nx, ny, nz) + 31) / 32) * sizeof(uint32_t);
}

// ---------------------------------------------------------------------------------------------------------------------- build
__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_build_kernel(int nx, int ny, int nz, int n_cells, int n_words,
                                                                            const float* __restrict__ vol, float threshold,
                                                                            int dilate, uint32_t* __restrict__ bits) {
  const int c = blockIdx.x * RSN_OCC_BLOCK + threadIdx.x;  // n_cells < 2^27: no overflow
  const int lane = threadIdx.x & 63;
  bool occ = false;
  if (c < n_cells) {
    const int cx = nx - 1, cy = ny - 1;
    const int i = c % cx, j = (c / cx) % cy, k = c / (cx * cy);
    const int i0 = max(i - dilate, 0), i1 = min(i + 1 + dilate, nx - 1);
    const int j0 = max(j - dilate, 0), j1 = min(j + 1 + dilate, ny - 1);
    const int k0 = max(k - dilate, 0), k1 = min(k + 1 + dilate, nz - 1);
    for (int kk = k0; kk <= k1; ++kk)
      for (int jj = j0; jj <= j1; ++jj) {
        const float* row = vol + ((size_t)kk * ny + jj) * nx;
        for (int ii = i0; ii <= i1; ++ii) occ = occ || !(row[ii] < threshold);  // NaN: occupied
      }
  }
  const unsigned long long bal = __ballot(occ);
  const int w = (c - lane) / 32 + (lane >> 5);  // the wave's first cell is a multiple of 64
  if ((lane & 31) == 0 && w < n_words) bits[w] = (uint32_t)(lane ? bal >> 32 : bal);
}

extern "C" int rsn_occupancy_build(int32_t nx, int32_t ny, int32_t nz, const float* vol, float threshold, int32_t dilate,
                                   uint32_t* bits, size_t bytes, void* stream) {
  RSN_REQUIRE(occ_dims_ok(nx, ny, nz), RSN_ERR_INVALID_ARGUMENT,
              "occupancy_build: grid %d x %d x %d: need every dimension >= 2 and nx*ny*nz <= 2^27", nx, ny, nz);
  RSN_REQUIRE(dilate >= 0 && dilate <= 2, RSN_ERR_INVALID_ARGUMENT, "occupancy_build: dilate=%d: need 0, 1 or 2", dilate);
  RSN_REQUIRE(vol && bits, RSN_ERR_INVALID_ARGUMENT, "occupancy_build: vol or bits is NULL");
  const int64_t cells = occ_cells(nx, ny, nz);
  const int64_t words = (cells + 31) / 32;
  RSN_REQUIRE(bytes >= (size_t)words * sizeof(uint32_t), RSN_ERR_INVALID_ARGUMENT,
              "occupancy_build: bits holds %zu bytes, the grid needs %zu", bytes, (size_t)words * sizeof(uint32_t));
  const unsigned blocks = (unsigned)((cells + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK);
  hipLaunchKernelGGL(rsn_occupancy_build_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, (hipStream_t)stream, nx, ny, nz,
                     (int)cells, (int)words, vol, threshold, dilate, bits);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// ----------------------------------------------------------------------------------------------------------------------- cull
struct OccGrid {
  int cx, cy, cz;         // cells per axis
  double org[3], inv[3];  // grid coordinate of a point p: (p - org) * inv
};

__device__ __forceinline__ bool occ_finite(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN and the infinities

// Does the segment o + t d, t in [near, far], cross an occupied cell (or, with outside_occupied, leave the box)?
__device__ bool occ_ray_hits(const OccGrid& g, const float* __restrict__ o3, const float* __restrict__ d3, float nearf, float farf,
                             const uint32_t* __restrict__ bits, bool outside_occupied) {
  bool ok = occ_finite(nearf) && occ_finite(farf) && farf >= nearf;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o3[a]) && occ_finite(d3[a]);
  if (!ok) return true;  // a ray that cannot be reasoned about is never culled
  const int cells[3] = {g.cx, g.cy, g.cz};
  double og[3], dg[3];
  double t0 = (double)nearf, t1 = (double)farf;
  bool leaves = false, empty = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    og[a] = ((double)o3[a] - g.org[a]) * g.inv[a];
    dg[a] = (double)d3[a] * g.inv[a];
    const double hi = (double)cells[a];
    const double pn = og[a] + (double)nearf * dg[a], pf = og[a] + (double)farf * dg[a];
    leaves = leaves || pn < 0.0 || pn > hi || pf < 0.0 || pf > hi;  // the box is convex: inside at both ends = inside throughout
    if (dg[a] == 0.0) {  // +0.0 and -0.0: parallel to the slab, no division
      empty = empty || og[a] < 0.0 || og[a] > hi;
    } else {
      const double ta = (0.0 - og[a]) / dg[a], tb = (hi - og[a]) / dg[a];
      t0 = fmax(t0, fmin(ta, tb));
      t1 = fmin(t1, fmax(ta, tb));
    }
  }
  if (outside_occupied && leaves) return true;
  if (empty || t0 > t1) return false;
  // the cell that holds the entry point, then one face crossing at a time until the exit parameter or the box's edge
  int idx[3], step[3];
  double tnext[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double p = og[a] + t0 * dg[a];
    int i = (int)floor(p);
    i = i < 0 ? 0 : (i > cells[a] - 1 ? cells[a] - 1 : i);
    idx[a] = i;
    step[a] = dg[a] > 0.0 ? 1 : (dg[a] < 0.0 ? -1 : 0);
    tnext[a] = step[a] == 0 ? INFINITY : ((double)(i + (step[a] > 0 ? 1 : 0)) - og[a]) / dg[a];
  }
  const int max_steps = g.cx + g.cy + g.cz;  // every step leaves a cell through one face, never to come back
  for (int s = 0; s <= max_steps; ++s) {
    const int c = (idx[2] * g.cy + idx[1]) * g.cx + idx[0];
    if ((bits[c >> 5] >> (c & 31)) & 1u) return true;
    const int a = tnext[0] <= tnext[1] ? (tnext[0] <= tnext[2] ? 0 : 2) : (tnext[1] <= tnext[2] ? 1 : 2);
    if (!(tnext[a] <= t1)) break;
    const int i = idx[a] + step[a];
    if (i < 0 || i >= cells[a]) break;
    idx[a] = i;
    tnext[a] = ((double)(i + (step[a] > 0 ? 1 : 0)) - og[a]) / dg[a];
  }
  return false;
}

__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_cull_kernel(int R, const float* __restrict__ origins,
                                                                           const float* __restrict__ directions,
                                                                           const float* __restrict__ nears,
                                                                           const float* __restrict__ fars, const OccGrid g,
                                                                           const uint32_t* __restrict__ bits, int outside_occupied,
                                                                           uint8_t* __restrict__ hit, int* __restrict__ block_counts) {
  __shared__ int s_wave_tot[RSN_OCC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = blockIdx.x * RSN_OCC_BLOCK + tid;
  bool h = false;
  if (r < R) {
    float o3[3], d3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o3[a] = origins[(size_t)r * 3 + a]; d3[a] = directions[(size_t)r * 3 + a]; }
    h = occ_ray_hits(g, o3, d3, nears[r], fars[r], bits, outside_occupied != 0);
    hit[r] = h ? 1 : 0;
  }
  const unsigned long long bal = __ballot(h);
  if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_OCC_BLOCK / 64; ++wv) t += s_wave_tot[wv];
    block_counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_index_kernel(int R, const uint8_t* __restrict__ hit,
                                                                            const int* __restrict__ block_counts,
                                                                            int* __restrict__ n_hit, int* __restrict__ ray_index) {
  __shared__ int s_wave_tot[RSN_OCC_BLOCK / 64];
  __shared__ int s_before[RSN_OCC_BLOCK / 64];
  __shared__ int s_all[RSN_OCC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // hit rays in the blocks in front of this one, and in all blocks
  int before = 0, all = 0;
  for (int j = tid; j < (int)gridDim.x; j += RSN_OCC_BLOCK) {
    const int v = block_counts[j];
    all += v;
    if (j < (int)blockIdx.x) before += v;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    before += __shfl_xor(before, off, 64);
    all += __shfl_xor(all, off, 64);
  }
  const int r = blockIdx.x * RSN_OCC_BLOCK + tid;
  const bool h = r < R && hit[r] != 0;
  const unsigned long long bal = __ballot(h);
  const int in_wave = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) {
    s_before[wid] = before;
    s_all[wid] = all;
    s_wave_tot[wid] = __builtin_popcountll(bal);
  }
  __syncthreads();
  int base = 0, total = 0, wave_off = 0;
#pragma unroll
  for (int wv = 0; wv < RSN_OCC_BLOCK / 64; ++wv) {
    base += s_before[wv];
    total += s_all[wv];
    if (wv < wid) wave_off += s_wave_tot[wv];
  }
  if (r < R) {
    const int hits_before = base + wave_off + in_wave;  // hit rays with a smaller index than r
    ray_index[h ? hits_before : total + (r - hits_before)] = r;
  }
  if (blockIdx.x == 0 && tid == 0) *n_hit = total;
}

extern "C" size_t rsn_occupancy_cull_workspace_bytes(int32_t n_rays) {
  return ((size_t)(n_rays > 0 ? n_rays : 0) + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK * sizeof(int32_t) + sizeof(int32_t);
}

extern "C" int rsn_occupancy_cull(int32_t n_rays, const float* origins, const float* directions, const float* nears,
                                  const float* fars, int32_t nx, int32_t ny, int32_t nz, const float* origin3,
                                  const float* spacing3, const uint32_t* bits, int32_t outside_occupied, uint8_t* hit,
                                  int32_t* n_hit, int32_t* ray_index, int32_t* workspace, void* stream) {
  RSN_REQUIRE(n_rays >= 0, RSN_ERR_INVALID_ARGUMENT, "occupancy_cull: n_rays=%d", n_rays);
  RSN_REQUIRE(occ_dims_ok(nx, ny, nz), RSN_ERR_INVALID_ARGUMENT,
              "occupancy_cull: grid %d x %d x %d: need every dimension >= 2 and nx*ny*nz <= 2^27", nx, ny, nz);
  RSN_REQUIRE(origin3 && spacing3, RSN_ERR_INVALID_ARGUMENT, "occupancy_cull: origin3 or spacing3 is NULL");
  OccGrid g;
  g.cx = nx - 1; g.cy = ny - 1; g.cz = nz - 1;
  for (int a = 0; a < 3; ++a) {
    RSN_REQUIRE(isfinite(origin3[a]) && isfinite(spacing3[a]) && spacing3[a] > 0.0f, RSN_ERR_INVALID_ARGUMENT,
                "occupancy_cull: axis %d: origin %g spacing %g: need finite values and spacing > 0", a, (double)origin3[a],
                (double)spacing3[a]);
    g.org[a] = (double)origin3[a];
    g.inv[a] = 1.0 / (double)spacing3[a];
  }
  RSN_REQUIRE(n_hit, RSN_ERR_INVALID_ARGUMENT, "occupancy_cull: n_hit is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (n_rays == 0) {
    RSN_HIP(hipMemsetAsync(n_hit, 0, sizeof(int32_t), st));
    return RSN_OK;
  }
  RSN_REQUIRE(origins && directions && nears && fars && bits && hit && ray_index && workspace, RSN_ERR_INVALID_ARGUMENT,
              "occupancy_cull: a pointer is NULL");
  const unsigned blocks = (unsigned)(((int64_t)n_rays + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK);
  hipLaunchKernelGGL(rsn_occupancy_cull_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, st, n_rays, origins, directions, nears,
                     fars, g, bits, outside_occupied, hit, workspace);
  hipLaunchKernelGGL(rsn_occupancy_index_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, st, n_rays, hit, workspace, n_hit,
                     ray_index);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// -------------------------------------------------------------------------------------------------------------------- scatter
#define RSN_SCATTER_MAX_BLOCKS 8192  // the rest of a large output is walked with a grid stride

__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_scatter_rows_kernel(int n_rows, const int* __restrict__ n_dev,
                                                                         const int* __restrict__ ray_index,
                                                                         const float* __restrict__ src, int row_floats, float fill,
                                                                         float* __restrict__ out) {
  int count = n_rows;
  if (n_dev) {
    const int nd = *n_dev;
    count = nd < 0 ? 0 : (nd < n_rows ? nd : n_rows);
  }
  const int64_t total = (int64_t)n_rows * row_floats;
  for (int64_t e = (int64_t)blockIdx.x * RSN_OCC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * RSN_OCC_BLOCK) {
    const int i = (int)(e / row_floats), c = (int)(e - (int64_t)i * row_floats);
    const int r = ray_index[i];
    if ((unsigned)r >= (unsigned)n_rows) continue;  // not a row of out: skipped rather than written through
    out[(int64_t)r * row_floats + c] = i < count ? src[e] : fill;
  }
}

extern "C" int rsn_scatter_rows(int32_t n_rows, const int32_t* n_dev, const int32_t* ray_index, const float* src,
                                int32_t row_floats, float fill, float* out, void* stream) {
  RSN_REQUIRE(n_rows >= 0 && row_floats >= 1, RSN_ERR_INVALID_ARGUMENT, "scatter_rows: n_rows=%d row_floats=%d", n_rows, row_floats);
  if (n_rows == 0) return RSN_OK;
  RSN_REQUIRE(ray_index && src && out, RSN_ERR_INVALID_ARGUMENT, "scatter_rows: a pointer is NULL");
  const int64_t want = ((int64_t)n_rows * row_floats + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK;
  const unsigned blocks = (unsigned)(want < RSN_SCATTER_MAX_BLOCKS ? want : RSN_SCATTER_MAX_BLOCKS);
  hipLaunchKernelGGL(rsn_scatter_rows_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, (hipStream_t)stream, n_rows, n_dev, ray_index,
                     src, row_floats, fill, out);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// -------------------------------------------------------------------------------------------------------------------- samples
#define RSN_OCC_PI 3.141592653589793

__device__ __forceinline__ int occ_count(const int* __restrict__ n_dev, int n) {
  if (!n_dev) return n;
  const int nd = *n_dev;
  return nd < 0 ? 0 : (nd < n ? nd : n);
}

// live[p] of sample p = r*S + i, and the number of live samples of every block
__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_mark_kernel(
    int R, const int* __restrict__ n_dev, int S, const float* __restrict__ origins, const float* __restrict__ directions,
    const float* __restrict__ pixel_area, const float* __restrict__ bins, const OccGrid g, const uint32_t* __restrict__ bits,
    int outside_occupied, float max_radius, uint8_t* __restrict__ live, int* __restrict__ block_counts) {
  __shared__ int s_wave_tot[RSN_OCC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int N = R * S;  // the launcher bounds it
  const int count = occ_count(n_dev, R);
  const int p = blockIdx.x * RSN_OCC_BLOCK + tid;
  bool l = false;
  if (p < N) {
    const int r = p / S, i = p - r * S;
    if (r < count) {  // the rays behind the count are never read
      float o3[3], d3[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) { o3[a] = origins[(size_t)r * 3 + a]; d3[a] = directions[(size_t)r * 3 + a]; }
      const float t0 = bins[(size_t)r * (S + 1) + i], t1 = bins[(size_t)r * (S + 1) + i + 1];
      const float pa = pixel_area[r];
      const double len = sqrt((double)d3[0] * d3[0] + (double)d3[1] * d3[1] + (double)d3[2] * d3[2]);
      // the cone's radius at the far end of the interval against the grid's margin; a NaN on the left compares false, and
      // whatever made it (a non-finite t or d) is flagged by occ_ray_hits
      l = !occ_finite(pa) || (double)t1 * len * sqrt((double)pa / RSN_OCC_PI) > (double)max_radius;
      l = l || occ_ray_hits(g, o3, d3, t0, t1, bits, outside_occupied != 0);
    }
    live[p] = l ? 1 : 0;
  }
  const unsigned long long bal = __ballot(l);
  if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_OCC_BLOCK / 64; ++wv) t += s_wave_tot[wv];
    block_counts[blockIdx.x] = t;
  }
}

// One workgroup: counts[b] -> the number of live samples in the blocks in front of b (in place), their total -> *n_live.
__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_scan_kernel(int n_blocks, int* __restrict__ counts, int* __restrict__ n_live) {
  __shared__ int s_wave_tot[RSN_OCC_BLOCK / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n_blocks; base += RSN_OCC_BLOCK) {  // the bound is the same in every lane
    const int j = base + tid;
    const int v = j < n_blocks ? counts[j] : 0;
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
    for (int wv = 0; wv < RSN_OCC_BLOCK / 64; ++wv) {
      const int t = s_wave_tot[wv];
      if (wv < wid) wave_off += t;
      tot += t;
    }
    const int carry = s_carry;
    if (j < n_blocks) counts[j] = carry + wave_off + x - v;
    __syncthreads();  // every lane has read s_carry and s_wave_tot
    if (tid == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (tid == 0) *n_live = s_carry;
}

__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_occupancy_compact_kernel(
    int R, int S, const float* __restrict__ origins, const float* __restrict__ directions, const float* __restrict__ pixel_area,
    const float* __restrict__ bins, const uint8_t* __restrict__ live, const int* __restrict__ block_offsets,
    const int* __restrict__ n_live, int* __restrict__ sample_index, float* __restrict__ origins_c, float* __restrict__ directions_c,
    float* __restrict__ pixel_area_c, float2* __restrict__ bins_c) {
  __shared__ int s_wave_tot[RSN_OCC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int N = R * S;
  const int p = blockIdx.x * RSN_OCC_BLOCK + tid;
  const bool l = p < N && live[p] != 0;
  const unsigned long long bal = __ballot(l);
  const int in_wave = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
  __syncthreads();
  int wave_off = 0;
#pragma unroll
  for (int wv = 0; wv < RSN_OCC_BLOCK / 64; ++wv)
    if (wv < wid) wave_off += s_wave_tot[wv];
  if (p >= N) return;
  const int before = block_offsets[blockIdx.x] + wave_off + in_wave;  // live samples with a smaller index than p: 0 .. p
  if (!l) {
    sample_index[*n_live + (p - before)] = p;  // total + the skipped samples in front of p: below N
    return;
  }
  sample_index[before] = p;
  const int r = p / S, i = p - r * S;
  const size_t j = (size_t)before;
#pragma unroll
  for (int a = 0; a < 3; ++a) {  // consecutive live lanes write consecutive rows
    origins_c[j * 3 + a] = origins[(size_t)r * 3 + a];
    directions_c[j * 3 + a] = directions[(size_t)r * 3 + a];
  }
  pixel_area_c[j] = pixel_area[r];
  bins_c[j] = make_float2(bins[(size_t)r * (S + 1) + i], bins[(size_t)r * (S + 1) + i + 1]);
}

static bool occ_samples_ok(int64_t n_rays, int64_t n_samples) {  // n_rays * n_samples * 3 <= INT32_MAX, without forming the product
  const int64_t most = (int64_t)INT32_MAX / 3;
  return n_rays >= 0 && n_samples >= 1 && n_samples <= most && n_rays <= most / n_samples;
}

extern "C" size_t rsn_occupancy_samples_workspace_bytes(int32_t n_rays, int32_t n_samples) {
  if (!occ_samples_ok(n_rays, n_samples)) {
    rsn_set_error("occupancy_samples: n_rays=%d n_samples=%d: need n_rays >= 0, n_samples >= 1 and n_rays*n_samples*3 < 2^31", n_rays,
                  n_samples);
    return 0;
  }
  const int64_t n = (int64_t)n_rays * n_samples;
  return (size_t)((n + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK + 1) * sizeof(int32_t);
}

extern "C" int rsn_occupancy_compact_samples(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* origins,
                                             const float* directions, const float* pixel_area, const float* euclid_bins, int32_t nx,
                                             int32_t ny, int32_t nz, const float* origin3, const float* spacing3, const uint32_t* bits,
                                             int32_t outside_occupied, float max_radius, uint8_t* live, int32_t* n_live,
                                             int32_t* sample_index, float* origins_c, float* directions_c, float* pixel_area_c,
                                             float* bins_c, int32_t* workspace, void* stream) {
  RSN_REQUIRE(occ_samples_ok(n_rays, n_samples), RSN_ERR_INVALID_ARGUMENT,
              "occupancy_compact_samples: n_rays=%d n_samples=%d: need n_rays >= 0, n_samples >= 1 and n_rays*n_samples*3 < 2^31", n_rays,
              n_samples);
  RSN_REQUIRE(occ_dims_ok(nx, ny, nz), RSN_ERR_INVALID_ARGUMENT,
              "occupancy_compact_samples: grid %d x %d x %d: need every dimension >= 2 and nx*ny*nz <= 2^27", nx, ny, nz);
  RSN_REQUIRE(origin3 && spacing3, RSN_ERR_INVALID_ARGUMENT, "occupancy_compact_samples: origin3 or spacing3 is NULL");
  OccGrid g;
  g.cx = nx - 1; g.cy = ny - 1; g.cz = nz - 1;
  for (int a = 0; a < 3; ++a) {
    RSN_REQUIRE(isfinite(origin3[a]) && isfinite(spacing3[a]) && spacing3[a] > 0.0f, RSN_ERR_INVALID_ARGUMENT,
                "occupancy_compact_samples: axis %d: origin %g spacing %g: need finite values and spacing > 0", a, (double)origin3[a],
                (double)spacing3[a]);
    g.org[a] = (double)origin3[a];
    g.inv[a] = 1.0 / (double)spacing3[a];
  }
  RSN_REQUIRE(!isnan(max_radius), RSN_ERR_INVALID_ARGUMENT, "occupancy_compact_samples: max_radius is NaN (+inf switches the rule off)");
  RSN_REQUIRE(n_live, RSN_ERR_INVALID_ARGUMENT, "occupancy_compact_samples: n_live is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (n_rays == 0) {
    RSN_HIP(hipMemsetAsync(n_live, 0, sizeof(int32_t), st));
    return RSN_OK;
  }
  RSN_REQUIRE(origins && directions && pixel_area && euclid_bins && bits && live && sample_index && origins_c && directions_c &&
                  pixel_area_c && bins_c && workspace,
              RSN_ERR_INVALID_ARGUMENT, "occupancy_compact_samples: a pointer is NULL");
  RSN_REQUIRE(((uintptr_t)bins_c & 7u) == 0, RSN_ERR_INVALID_ARGUMENT, "occupancy_compact_samples: bins_c must be 8-byte aligned");
  const int64_t n = (int64_t)n_rays * n_samples;
  const unsigned blocks = (unsigned)((n + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK);
  hipLaunchKernelGGL(rsn_occupancy_mark_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, st, n_rays, n_dev, n_samples, origins, directions,
                     pixel_area, euclid_bins, g, bits, outside_occupied, max_radius, live, workspace);
  hipLaunchKernelGGL(rsn_occupancy_scan_kernel, dim3(1), dim3(RSN_OCC_BLOCK), 0, st, (int)blocks, workspace, n_live);
  hipLaunchKernelGGL(rsn_occupancy_compact_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, st, n_rays, n_samples, origins, directions,
                     pixel_area, euclid_bins, live, workspace, n_live, sample_index, origins_c, directions_c, pixel_area_c,
                     (float2*)bins_c);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// One launch for every member of a level: compact row j -> row sample_index[j], zeros in the rows of the skipped samples.
#define RSN_LEVEL_MEMBERS 9
struct OccLevel {
  const float* src[RSN_LEVEL_MEMBERS];
  float* dst[RSN_LEVEL_MEMBERS];
  int wide[RSN_LEVEL_MEMBERS];  // rows of three floats (else of one)
};

__global__ __launch_bounds__(RSN_OCC_BLOCK) void rsn_scatter_level_kernel(int n, const int* __restrict__ n_live,
                                                                          const int* __restrict__ sample_index, const OccLevel L) {
  const int nl = occ_count(n_live, n);
  for (int64_t j = (int64_t)blockIdx.x * RSN_OCC_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * RSN_OCC_BLOCK) {
    const int p = sample_index[j];
    if ((unsigned)p >= (unsigned)n) continue;  // not a row of dst: skipped rather than written through
    const bool l = j < nl;                     // rows of src at and past the count are never read
#pragma unroll
    for (int m = 0; m < RSN_LEVEL_MEMBERS; ++m) {
      if (!L.dst[m]) continue;  // the same in every lane
      if (L.wide[m]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) L.dst[m][(size_t)p * 3 + c] = l ? L.src[m][(size_t)j * 3 + c] : 0.0f;
      } else {
        L.dst[m][p] = l ? L.src[m][j] : 0.0f;
      }
    }
  }
}

extern "C" int rsn_scatter_level(int32_t n_points, const int32_t* n_live, const int32_t* sample_index, const rsn_field_outputs* src,
                                 const rsn_field_outputs* dst, void* stream) {
  RSN_REQUIRE(n_points >= 0 && (int64_t)n_points * 3 <= (int64_t)INT32_MAX, RSN_ERR_INVALID_ARGUMENT,
              "scatter_level: n_points=%d: need 0 <= n_points and n_points*3 < 2^31", n_points);
  RSN_REQUIRE(src && dst, RSN_ERR_INVALID_ARGUMENT, "scatter_level: src or dst is NULL");
  float* const s[RSN_LEVEL_MEMBERS] = {src->sigma, src->color, src->pred_normals, src->n_dot_d, src->diff, src->tint, src->roughness,
                                       src->raw_density, src->raw_roughness};
  float* const d[RSN_LEVEL_MEMBERS] = {dst->sigma, dst->color, dst->pred_normals, dst->n_dot_d, dst->diff, dst->tint, dst->roughness,
                                       dst->raw_density, dst->raw_roughness};
  static const int wide[RSN_LEVEL_MEMBERS] = {0, 1, 1, 0, 1, 1, 0, 0, 0};
  OccLevel L;
  int members = 0;
  for (int m = 0; m < RSN_LEVEL_MEMBERS; ++m) {
    RSN_REQUIRE((s[m] != nullptr) == (d[m] != nullptr), RSN_ERR_INVALID_ARGUMENT,
                "scatter_level: member %d is set in one of src / dst and NULL in the other", m);
    L.src[m] = s[m];
    L.dst[m] = d[m];
    L.wide[m] = wide[m];
    members += s[m] != nullptr;
  }
  if (n_points == 0 || members == 0) return RSN_OK;
  RSN_REQUIRE(n_live && sample_index, RSN_ERR_INVALID_ARGUMENT, "scatter_level: n_live or sample_index is NULL");
  const int64_t want = ((int64_t)n_points + RSN_OCC_BLOCK - 1) / RSN_OCC_BLOCK;
  const unsigned blocks = (unsigned)(want < RSN_SCATTER_MAX_BLOCKS ? want : RSN_SCATTER_MAX_BLOCKS);
  hipLaunchKernelGGL(rsn_scatter_level_kernel, dim3(blocks), dim3(RSN_OCC_BLOCK), 0, (hipStream_t)stream, n_points, n_live,
                     sample_index, L);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
