// Multi-scale data path (include/rsn.h, "image pyramids"):
//   rsn_build_pyramid        levels 1 .. L-1 of every image as white-blended fp32 box averages of level 0, one lane per output pixel
//   rsn_sample_pyramid_rays  Philox level + pixel sampler, pixel gather and camera ray generator, one lane per ray
//   rsn_sample_capture_rays  the same sampler with a camera table: per-image intrinsics and lens distortion (rsn_camera.h capture_ray)
//   rsn_sample_capture_rays_live  the same again with a 9- or 12-column table (fisheye rows) and the pixel drawn from live-pixel lists
// Level 0 is the uint8 RGBA image set itself and is never copied.  Recipes: include/rsn.h.
#include "rsn_camera.h"
#include "rsn_common.h"
#include "rsn_philox.h"

namespace {

constexpr int MAX_LEVELS = RSN_PYRAMID_MAX_LEVELS;

// off[l] = first pixel of level l inside the pyramid allocation, l = 1 .. L-1 (levels in order, within a level image after image);
// off[L] = its size in pixels; off[0] is unused (level 0 lives in `images`)
struct LevelTable {
  uint32_t off[MAX_LEVELS + 1];
};

// N*H*W < 2^32 (checked by the host) bounds every level and the pyramid (the levels l >= 1 together hold < N*H*W / 3 pixels)
inline LevelTable level_table(int32_t n_images, int32_t height, int32_t width, int32_t levels) {
  LevelTable t{};
  uint64_t at = 0;
  for (int l = 1; l <= levels; ++l) {
    t.off[l] = (uint32_t)at;
    if (l < levels) at += (uint64_t)n_images * (uint64_t)(height >> l) * (uint64_t)(width >> l);
  }
  return t;
}

// ------------------------------------------------------------------------------------------------ pyramid
struct PyramidArgs {
  int32_t n_images, height, width, levels;
  const uint8_t* images;  // [N, H, W, 4]
  float* pyramid;         // [off[L], 3]
  LevelTable t;
};

// One launch for all levels: lane p owns pixel p of the allocation and finds its level in the table (three compares; a wave
// straddles a level boundary at most once per level).  Against one launch per level (tools/probes/pyramid_launch_probe.hip, 100
// images of 800 x 800): 0.319 ms against 0.329 ms at four levels, 0.547 ms against 0.454 ms at five.
__global__ __launch_bounds__(256) void rsn_build_pyramid_kernel(PyramidArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.t.off[a.levels]) return;
  int l = 1;
  uint32_t first = a.t.off[1];
#pragma unroll
  for (int k = 2; k < MAX_LEVELS; ++k)  // static indices: the table stays in scalar registers
    if (k < a.levels && p >= a.t.off[k]) {
      l = k;
      first = a.t.off[k];
    }
  const uint32_t wl = (uint32_t)(a.width >> l), hwl = (uint32_t)(a.height >> l) * wl;
  const uint32_t local = p - first;
  const uint32_t i = local / hwl, rem = local - i * hwl;
  const uint32_t Y = rem / wl, X = rem - Y * wl;
  const int s = 1 << l;
  const uchar4* src = reinterpret_cast<const uchar4*>(a.images) +
                      ((size_t)i * (size_t)a.height + (size_t)Y * s) * (size_t)a.width + (size_t)X * s;
  uint32_t S[3] = {0u, 0u, 0u};
  for (int dy = 0; dy < s; ++dy) {
    for (int dx = 0; dx < s; ++dx) {
      const uchar4 px = src[dx];
      const uint32_t a8 = px.w, white = 255u * (255u - a8);
      S[0] += (uint32_t)px.x * a8 + white;
      S[1] += (uint32_t)px.y * a8 + white;
      S[2] += (uint32_t)px.z * a8 + white;
    }
    src += a.width;
  }
  const float den = (float)(65025u * (uint32_t)(s * s));  // <= 16,646,400 < 2^24, like every S: both exact
#pragma unroll
  for (int j = 0; j < 3; ++j) a.pyramid[(size_t)p * 3 + j] = (float)S[j] / den;
}

// ------------------------------------------------------------------------------------------------ sampler
struct PyramidSampleArgs {
  int32_t n_images, height, width, levels, n_rays;
  const uint8_t* images;  // [N, H, W, 4]
  const float* pyramid;   // [off[L], 3]; not read when levels == 1
  const float* c2w;       // [N, 3, 4]
  Intrinsics k;           // the one camera of all images (CAPTURE: not read)
  const float* cameras;   // CAPTURE: the camera table [N, 9] (else not read); LIVE: [N, camera_stride]
  int32_t camera_stride;  // LIVE: 9 or 12
  const uint32_t* live;   // LIVE: the levels' live-pixel lists, or NULL: every pixel
  const uint32_t* live_offsets;  // LIVE: [levels + 1], level l's list is live[live_offsets[l] .. live_offsets[l+1]) (not read without live)
  uint32_t seed, rank, step;
  float* origins;
  float* directions;
  float* pixel_area;
  float* rgb;
  int32_t* indices;
  int32_t* level;
  LevelTable t;
};

// CAPTURE: image i's camera is row i of a.cameras, and the ray comes from capture_ray, which is camera_ray for a row without
// distortion.  LIVE: the flat pixel is drawn from the level's live-pixel list, the row has a.camera_stride columns and a fisheye row
// takes fisheye_ray (rsn_camera.h lens_ray).  Everything else -- the Philox draw, the gather, the blend, the outputs -- is one text.
enum SampleMode { PINHOLE = 0, CAPTURE = 1, LIVE = 2 };

template <SampleMode MODE>
__global__ __launch_bounds__(256) void rsn_sample_pyramid_rays_kernel(PyramidSampleArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_rays) return;
  const U4 rnd = philox4x32_10(U4{a.step, (uint32_t)r, 0u, 0u}, a.seed, a.rank);
  const int l = (int)(((uint64_t)rnd.y * (uint32_t)a.levels) >> 32);
  const uint32_t wl = (uint32_t)(a.width >> l), hw = (uint32_t)(a.height >> l) * wl;
  const uint32_t total = hw * (uint32_t)a.n_images;  // < 2^32 (checked by the host for level 0, the largest)
  uint32_t flat = (uint32_t)(((uint64_t)rnd.x * total) >> 32);
  if (MODE == LIVE && a.live) {
    const uint32_t first = a.live_offsets[l], count = a.live_offsets[l + 1] - first;
    // a level without a live pixel is the caller's error (the data manager refuses it): pixel 0 then, and never a read outside
    // `live`; the clamp keeps a list that is not one of this image set from indexing outside the images
    flat = count ? min(a.live[first + (uint32_t)(((uint64_t)rnd.x * count) >> 32)], total - 1u) : 0u;
  }
  const int i = (int)(flat / hw);
  const uint32_t rem = flat - (uint32_t)i * hw;
  const int y = (int)(rem / wl), x = (int)(rem - (uint32_t)y * wl);
  const float inv = 1.0f / (float)(1 << l);  // a power of two: the level's intrinsics are exact
  float o[3], d[3], area;
  if (MODE == LIVE) {
    LensCamera lc = load_lens_camera(a.cameras + (size_t)i * (size_t)a.camera_stride, a.camera_stride);
    lc.c.k = Intrinsics{lc.c.k.fx * inv, lc.c.k.fy * inv, lc.c.k.cx * inv, lc.c.k.cy * inv};
    lens_ray(a.c2w + (size_t)i * 12, lc, y, x, o, d, &area);
  } else if (MODE == CAPTURE) {  // the coefficients act on normalised coordinates: a level changes the four intrinsics only
    Camera c = load_camera(a.cameras + (size_t)i * 9);
    c.k = Intrinsics{c.k.fx * inv, c.k.fy * inv, c.k.cx * inv, c.k.cy * inv};
    capture_ray(a.c2w + (size_t)i * 12, c, y, x, o, d, &area);
  } else {
    const Intrinsics k{a.k.fx * inv, a.k.fy * inv, a.k.cx * inv, a.k.cy * inv};
    camera_ray(a.c2w + (size_t)i * 12, k, y, x, o, d, &area);
  }
  float c[3];
  if (l == 0) {  // today's blend (rsn_sample_camera_rays)
    const uchar4 px = reinterpret_cast<const uchar4*>(a.images)[(size_t)flat];
    const float alpha = (float)px.w / 255.0f;
    const float c8[3] = {(float)px.x / 255.0f, (float)px.y / 255.0f, (float)px.z / 255.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = c8[j] * alpha + (1.0f - alpha);
  } else {
    uint32_t first = a.t.off[1];
#pragma unroll
    for (int k = 2; k < MAX_LEVELS; ++k)
      if (l == k) first = a.t.off[k];
    const float* px = a.pyramid + ((size_t)first + flat) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = px[j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a.origins[3 * r + j] = o[j];
    a.directions[3 * r + j] = d[j];
    a.rgb[3 * r + j] = c[j];
  }
  a.pixel_area[r] = area;
  a.indices[3 * r + 0] = i;
  a.indices[3 * r + 1] = y;
  a.indices[3 * r + 2] = x;
  if (a.level) a.level[r] = l;  // NULL only from the capture sampler at levels == 1, where every level is 0
}

// the checks both calls share; the message names what was given
int check_pyramid_shape(int32_t n_images, int32_t height, int32_t width, int32_t levels) {
  RSN_REQUIRE(levels >= 1 && levels <= MAX_LEVELS, RSN_ERR_INVALID_ARGUMENT,
              "levels=%d: 1 to %d (a box of 16 x 16 pixels keeps the integer sums below 2^24)", levels, MAX_LEVELS);
  RSN_REQUIRE(n_images >= 1 && height >= 1 && width >= 1, RSN_ERR_INVALID_ARGUMENT, "n_images=%d height=%d width=%d", n_images,
              height, width);
  const int32_t s = 1 << (levels - 1);
  RSN_REQUIRE(height % s == 0 && width % s == 0, RSN_ERR_INVALID_ARGUMENT,
              "height=%d width=%d: levels=%d needs both divisible by 2^(levels-1) = %d", height, width, levels, s);
  RSN_REQUIRE((uint64_t)n_images * (uint64_t)height * (uint64_t)width < (1ull << 32), RSN_ERR_INVALID_ARGUMENT,
              "n_images*height*width = %llu pixels: at most 2^32 - 1", (unsigned long long)n_images * height * width);
  return RSN_OK;
}

// all samplers: the checks, the level table, one launch.  CAPTURE and LIVE: the camera table `cameras`, else the shared pinhole k;
// LIVE: the table's stride and the live-pixel lists
int sample_rays(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images, const float* pyramid,
                size_t pyramid_pixels, const float* c2w, SampleMode mode, Intrinsics k, const float* cameras, int32_t camera_stride,
                const uint32_t* live, const uint32_t* live_offsets, int32_t n_rays,
                uint32_t seed, uint32_t rank, uint32_t step, float* origins, float* directions, float* pixel_area, float* rgb, int32_t* indices,
                int32_t* level, void* stream) {
  RSN_TRY(check_pyramid_shape(n_images, height, width, levels));
  RSN_REQUIRE(n_rays >= 0, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  const bool capture = mode != PINHOLE;
  RSN_REQUIRE(mode != LIVE || camera_stride == 9 || camera_stride == 12, RSN_ERR_INVALID_ARGUMENT, "camera_stride=%d: 9 or 12",
              camera_stride);
  RSN_REQUIRE(!live || (live_offsets && (((uintptr_t)live | (uintptr_t)live_offsets) & 3u) == 0), RSN_ERR_INVALID_ARGUMENT,
              "live needs live_offsets, both 4-byte aligned");
  RSN_REQUIRE(capture || (k.fx != 0.0f && k.fy != 0.0f), RSN_ERR_INVALID_ARGUMENT, "fx=%g fy=%g", (double)k.fx, (double)k.fy);
  if (n_rays == 0) return RSN_OK;
  RSN_REQUIRE(images && c2w && origins && directions && pixel_area && rgb && indices && (level || (capture && levels == 1)) &&
                  (pyramid || levels == 1) && (cameras || !capture),
              RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  RSN_REQUIRE(((uintptr_t)images & 3) == 0, RSN_ERR_INVALID_ARGUMENT, "images must be 4-byte aligned");
  const LevelTable t = level_table(n_images, height, width, levels);
  RSN_REQUIRE(pyramid_pixels >= t.off[levels], RSN_ERR_INVALID_ARGUMENT, "pyramid of %zu pixels, %u needed", pyramid_pixels,
              t.off[levels]);
  PyramidSampleArgs a{n_images, height, width, levels, n_rays, images, pyramid, c2w, k, cameras, camera_stride, live, live_offsets,
                      seed, rank, step, origins, directions, pixel_area, rgb, indices, level, t};
  const dim3 grid((unsigned)((n_rays + 255) / 256));
  if (mode == LIVE)
    hipLaunchKernelGGL(rsn_sample_pyramid_rays_kernel<LIVE>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (mode == CAPTURE)
    hipLaunchKernelGGL(rsn_sample_pyramid_rays_kernel<CAPTURE>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rsn_sample_pyramid_rays_kernel<PINHOLE>, grid, dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

}  // namespace

extern "C" int rsn_build_pyramid(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                                 float* pyramid, size_t pyramid_pixels, void* stream) {
  RSN_TRY(check_pyramid_shape(n_images, height, width, levels));
  const LevelTable t = level_table(n_images, height, width, levels);
  const uint32_t need = t.off[levels];
  if (need == 0) return RSN_OK;  // levels == 1: level 0 is the image set itself
  RSN_REQUIRE(images && pyramid, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  RSN_REQUIRE(((uintptr_t)images & 3) == 0, RSN_ERR_INVALID_ARGUMENT, "images must be 4-byte aligned");
  RSN_REQUIRE(pyramid_pixels >= need, RSN_ERR_INVALID_ARGUMENT, "pyramid of %zu pixels, %u needed", pyramid_pixels, need);
  PyramidArgs a{n_images, height, width, levels, images, pyramid, t};
  hipLaunchKernelGGL(rsn_build_pyramid_kernel, dim3((need + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_sample_pyramid_rays(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                                       const float* pyramid, size_t pyramid_pixels, const float* c2w, float fx, float fy, float cx, float cy,
                                       int32_t n_rays, uint32_t seed, uint32_t rank, uint32_t step, float* origins,
                                       float* directions, float* pixel_area, float* rgb, int32_t* indices, int32_t* level,
                                       void* stream) {
  return sample_rays(n_images, height, width, levels, images, pyramid, pyramid_pixels, c2w, PINHOLE, Intrinsics{fx, fy, cx, cy}, nullptr,
                     0, nullptr, nullptr, n_rays, seed, rank, step, origins, directions, pixel_area, rgb, indices, level, stream);
}

extern "C" int rsn_sample_capture_rays(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                                       const float* pyramid, size_t pyramid_pixels, const float* c2w, const float* cameras,
                                       int32_t n_rays, uint32_t seed, uint32_t rank, uint32_t step, float* origins,
                                       float* directions, float* pixel_area, float* rgb, int32_t* indices, int32_t* level,
                                       void* stream) {
  return sample_rays(n_images, height, width, levels, images, pyramid, pyramid_pixels, c2w, CAPTURE, Intrinsics{}, cameras, 9, nullptr,
                     nullptr, n_rays,
                     seed, rank, step, origins, directions, pixel_area, rgb, indices, level, stream);
}

extern "C" int rsn_sample_capture_rays_live(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                                            const float* pyramid, size_t pyramid_pixels, const float* c2w, const float* cameras,
                                            int32_t camera_stride, const uint32_t* live, const uint32_t* live_offsets, int32_t n_rays,
                                            uint32_t seed, uint32_t rank, uint32_t step, float* origins, float* directions,
                                            float* pixel_area, float* rgb, int32_t* indices, int32_t* level, void* stream) {
  return sample_rays(n_images, height, width, levels, images, pyramid, pyramid_pixels, c2w, LIVE, Intrinsics{}, cameras, camera_stride,
                     live, live_offsets, n_rays, seed, rank, step, origins, directions, pixel_area, rgb, indices, level, stream);
}
