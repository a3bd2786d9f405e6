// Live-pixel lists of a masked image set (include/rsn.h, "captures: masks and fisheye lenses"):
//   rsn_build_live_pixels   for every pyramid level the ascending list of the flat level-pixel indices that may be trained on
// A level-l pixel is live when all 2^l x 2^l level-0 pixels under it are.  Stable compaction without atomics, the scheme of
// rsn_pointcloud_select: (1) the live count of every tile of 256 level pixels; (2) one workgroup per level turns its tiles' counts
// into the number of live pixels in front of each tile, and writes the level's total; (3) every tile writes its live indices behind
// that number, a lane's place within the tile from ballots.  (1) and (3) evaluate the same predicate on the same bytes, so the list
// is identical from run to run and equal to numpy's flatnonzero.
#include "rsn_common.h"

namespace {

constexpr int MAX_LEVELS = RSN_PYRAMID_MAX_LEVELS;
constexpr int BLOCK = RSN_LIVE_TILE;  // level pixels per tile = lanes per workgroup
static_assert(RSN_LIVE_SCAN_CHUNK == BLOCK * BLOCK, "one trip of the scan's loop covers BLOCK tiles");

struct LiveArgs {
  int32_t n_images, height, width, levels;
  const uint8_t* masks;               // [N, H, W], non-zero = live
  uint32_t tile_first[MAX_LEVELS + 1];  // the first tile of level l; [levels] = the number of tiles
};

// N*H*W < 2^32 (checked by the host), so every level's pixel count fits 32 bits and the tile counts sum below 2^25
inline uint64_t level_pixels(int32_t n_images, int32_t height, int32_t width, int l) {
  return (uint64_t)n_images * (uint64_t)(height >> l) * (uint64_t)(width >> l);
}

inline void tile_table(LiveArgs& a) {
  uint64_t at = 0;
  for (int l = 0; l <= MAX_LEVELS; ++l) {
    a.tile_first[l] = (uint32_t)at;
    if (l < a.levels) at += (level_pixels(a.n_images, a.height, a.width, l) + BLOCK - 1) / BLOCK;
  }
}

// this workgroup's level, and whether this lane's level pixel q exists and is live
__device__ __forceinline__ bool live_here(const LiveArgs& a, int* level, uint32_t* tile, uint32_t* q) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k)  // static indices: the table stays in scalar registers
    if (k < a.levels && blockIdx.x >= a.tile_first[k]) l = k;
  uint32_t first = a.tile_first[0];
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k)
    if (l == k) first = a.tile_first[k];
  const uint32_t wl = (uint32_t)(a.width >> l), hwl = (uint32_t)(a.height >> l) * wl;
  const uint64_t q64 = (uint64_t)(blockIdx.x - first) * BLOCK + threadIdx.x;
  *level = l;
  *tile = blockIdx.x;
  *q = (uint32_t)q64;
  if (q64 >= (uint64_t)hwl * (uint32_t)a.n_images) return false;
  const uint32_t i = *q / hwl, rem = *q - i * hwl;
  const uint32_t Y = rem / wl, X = rem - Y * wl;
  const int s = 1 << l;
  const uint8_t* src = a.masks + ((size_t)i * (size_t)a.height + (size_t)Y * s) * (size_t)a.width + (size_t)X * s;
  bool live = true;
  for (int dy = 0; dy < s; ++dy) {
    for (int dx = 0; dx < s; ++dx) live = live && src[dx] != 0;
    src += a.width;
  }
  return live;
}

__global__ __launch_bounds__(BLOCK) void rsn_live_count_kernel(const LiveArgs a, uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_wave_tot[BLOCK / 64];
  int l;
  uint32_t tile, q;
  const bool live = live_here(a, &l, &tile, &q);
  const unsigned long long bal = __ballot(live);
  if ((threadIdx.x & 63) == 0) s_wave_tot[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int wv = 0; wv < BLOCK / 64; ++wv) t += s_wave_tot[wv];
    tile_counts[tile] = t;
  }
}

// Workgroup l: the counts of level l's tiles -> the number of live pixels in the tiles in front of each (in place), BLOCK tiles
// (RSN_LIVE_SCAN_CHUNK pixels) per trip with the running total carried from trip to trip; the level's total -> counts[l].
__global__ __launch_bounds__(BLOCK) void rsn_live_scan_kernel(const LiveArgs a, uint32_t* __restrict__ tile_counts,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_wave_tot[BLOCK / 64];
  __shared__ uint32_t s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t first = a.tile_first[0], end = a.tile_first[1];
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k)
    if ((int)blockIdx.x == k) first = a.tile_first[k], end = a.tile_first[k + 1];
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (uint32_t base = first; base < end; base += BLOCK) {  // the bound is the same in every lane
    const uint32_t j = base + tid;
    const uint32_t v = j < end ? tile_counts[j] : 0u;
    uint32_t x = v;  // inclusive scan of the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_wave_tot[wid] = x;
    __syncthreads();
    uint32_t wave_off = 0, tot = 0;
#pragma unroll
    for (int wv = 0; wv < BLOCK / 64; ++wv) {
      const uint32_t t = s_wave_tot[wv];
      if (wv < wid) wave_off += t;
      tot += t;
    }
    const uint32_t carry = s_carry;
    if (j < end) tile_counts[j] = carry + wave_off + x - v;
    __syncthreads();  // every lane has read s_carry and s_wave_tot
    if (tid == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = s_carry;
}

__global__ __launch_bounds__(BLOCK) void rsn_live_emit_kernel(const LiveArgs a, const uint32_t* __restrict__ tile_offsets,
                                                              const uint32_t* __restrict__ counts, uint32_t* __restrict__ live_out,
                                                              size_t live_capacity) {
  __shared__ uint32_t s_wave_tot[BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int l;
  uint32_t tile, q;
  const bool live = live_here(a, &l, &tile, &q);  // as in the count pass: the same function on the same bytes
  const unsigned long long bal = __ballot(live);
  const uint32_t in_wave = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave_tot[wid] = (uint32_t)__builtin_popcountll(bal);
  __syncthreads();
  if (!live) return;
  uint32_t wave_off = 0;
#pragma unroll
  for (int wv = 0; wv < BLOCK / 64; ++wv)
    if (wv < wid) wave_off += s_wave_tot[wv];
  size_t level_first = 0;  // the lists of the levels in front of this one
#pragma unroll
  for (int k = 0; k < MAX_LEVELS - 1; ++k)
    if (k < l) level_first += counts[k];
  const size_t row = level_first + tile_offsets[tile] + wave_off + in_wave;  // live pixels with a smaller index, all levels in front
  if (row < live_capacity) live_out[row] = q;  // never a byte past the capacity
}

int check_live_shape(int32_t n_images, int32_t height, int32_t width, int32_t levels) {
  RSN_REQUIRE(levels >= 1 && levels <= MAX_LEVELS, RSN_ERR_INVALID_ARGUMENT, "live pixels: levels=%d: 1 to %d", levels, MAX_LEVELS);
  RSN_REQUIRE(n_images >= 1 && height >= 1 && width >= 1, RSN_ERR_INVALID_ARGUMENT, "live pixels: n_images=%d height=%d width=%d",
              n_images, height, width);
  const int32_t s = 1 << (levels - 1);
  RSN_REQUIRE(height % s == 0 && width % s == 0, RSN_ERR_INVALID_ARGUMENT,
              "live pixels: height=%d width=%d: levels=%d needs both divisible by 2^(levels-1) = %d", height, width, levels, s);
  RSN_REQUIRE((uint64_t)n_images * (uint64_t)height * (uint64_t)width < (1ull << 32), RSN_ERR_INVALID_ARGUMENT,
              "live pixels: n_images*height*width = %llu pixels: at most 2^32 - 1", (unsigned long long)n_images * height * width);
  return RSN_OK;
}

}  // namespace

extern "C" size_t rsn_live_pixels_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t levels) {
  if (check_live_shape(n_images, height, width, levels) != RSN_OK) return 0;
  LiveArgs a{n_images, height, width, levels, nullptr, {}};
  tile_table(a);
  return (size_t)a.tile_first[levels] * sizeof(uint32_t);
}

extern "C" int rsn_build_live_pixels(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* masks,
                                     uint32_t* live, size_t live_capacity, uint32_t* counts, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  RSN_TRY(check_live_shape(n_images, height, width, levels));
  RSN_REQUIRE(masks && counts && workspace, RSN_ERR_INVALID_ARGUMENT, "live pixels: masks, counts or workspace is NULL");
  RSN_REQUIRE(((uintptr_t)workspace & 3u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)live & 3u) == 0,
              RSN_ERR_INVALID_ARGUMENT, "live pixels: live, counts and workspace must be 4-byte aligned");
  LiveArgs a{n_images, height, width, levels, masks, {}};
  tile_table(a);
  const size_t need = (size_t)a.tile_first[levels] * sizeof(uint32_t);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "live pixels: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  uint32_t* tile_counts = (uint32_t*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rsn_live_count_kernel, dim3(a.tile_first[levels]), dim3(BLOCK), 0, st, a, tile_counts);
  RSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(rsn_live_scan_kernel, dim3((unsigned)levels), dim3(BLOCK), 0, st, a, tile_counts, counts);
  RSN_HIP(hipGetLastError());
  if (live && live_capacity > 0) {
    hipLaunchKernelGGL(rsn_live_emit_kernel, dim3(a.tile_first[levels]), dim3(BLOCK), 0, st, a, tile_counts, counts, live,
                       live_capacity);
    RSN_HIP(hipGetLastError());
  }
  return RSN_OK;
}
