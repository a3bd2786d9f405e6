// The standalone data path (reference reflect_sampling_nerf_datamanager.py:49-58 next_train, model.py:468-479 metrics):
//   rsn_sample_camera_rays  Philox pixel sampler + pixel gather + camera ray generator, one thread per ray
//   rsn_camera_rays_image   the same ray arithmetic for every pixel of one camera (rendering views)
//   rsn_capture_rays_image  every pixel of one camera of a capture: a camera-table row with lens distortion (rsn_camera.h capture_ray)
//   rsn_capture_rays_image2 the same for a row of 9 or 12 columns: a fisheye row takes the equidistant model (rsn_camera.h lens_ray)
//   rsn_gather_ray_depth    the target distance along the ray of every sampled pixel, from a capture's depth maps (depth supervision)
//   rsn_ssim                torchmetrics' structural_similarity_index_measure of two [H, W, 3] images, on the device
// Recipes (Philox keying, ray arithmetic, SSIM definition): include/rsn.h.
#include "rsn_camera.h"
#include "rsn_common.h"
#include "rsn_philox.h"

namespace {

// ------------------------------------------------------------------------------------------------ camera rays
// Intrinsics and camera_ray: rsn_camera.h (shared with rsn_pointcloud.hip and rsn_pyramid.hip); Philox4x32-10: rsn_philox.h
struct SampleArgs {
  int32_t n_images, height, width, n_rays;
  const uint8_t* images;  // [N, H, W, 4]
  const float* c2w;       // [N, 3, 4]
  Intrinsics k;
  uint32_t seed, rank, step;
  float* origins;
  float* directions;
  float* pixel_area;
  float* rgb;
  int32_t* indices;
};

__global__ __launch_bounds__(256) void rsn_sample_camera_rays_kernel(SampleArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_rays) return;
  const U4 rnd = philox4x32_10(U4{a.step, (uint32_t)r, 0u, 0u}, a.seed, a.rank);
  const uint32_t hw = (uint32_t)a.height * (uint32_t)a.width;
  const uint32_t total = hw * (uint32_t)a.n_images;  // < 2^32 (checked by the host)
  const uint32_t flat = (uint32_t)(((uint64_t)rnd.x * total) >> 32);
  const int i = (int)(flat / hw);
  const uint32_t rem = flat - (uint32_t)i * hw;
  const int y = (int)(rem / (uint32_t)a.width), x = (int)(rem - (uint32_t)y * (uint32_t)a.width);
  float o[3], d[3], area;
  camera_ray(a.c2w + (size_t)i * 12, a.k, y, x, o, d, &area);
  const uchar4 px = reinterpret_cast<const uchar4*>(a.images)[(size_t)flat];
  const float alpha = (float)px.w / 255.0f;
  const float c[3] = {(float)px.x / 255.0f, (float)px.y / 255.0f, (float)px.z / 255.0f};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a.origins[3 * r + j] = o[j];
    a.directions[3 * r + j] = d[j];
    a.rgb[3 * r + j] = c[j] * alpha + (1.0f - alpha);  // RGBRenderer.blend_background, white
  }
  a.pixel_area[r] = area;
  a.indices[3 * r + 0] = i;
  a.indices[3 * r + 1] = y;
  a.indices[3 * r + 2] = x;
}

__global__ __launch_bounds__(256) void rsn_camera_rays_image_kernel(int height, int width, const float* c2w, Intrinsics k,
                                                                    float* origins, float* directions, float* pixel_area) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= height * width) return;
  const int y = p / width, x = p - y * width;
  float o[3], d[3], area;
  camera_ray(c2w, k, y, x, o, d, &area);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    origins[3 * p + j] = o[j];
    directions[3 * p + j] = d[j];
  }
  pixel_area[p] = area;
}

// the camera row is read on the device: no host read, and a caller may pass a row of a table it scaled there
__global__ __launch_bounds__(256) void rsn_capture_rays_image_kernel(int height, int width, const float* c2w, const float* camera,
                                                                     float* origins, float* directions, float* pixel_area) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= height * width) return;
  const int y = p / width, x = p - y * width;
  float o[3], d[3], area;
  capture_ray(c2w, load_camera(camera), y, x, o, d, &area);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    origins[3 * p + j] = o[j];
    directions[3 * p + j] = d[j];
  }
  pixel_area[p] = area;
}

// a row of a 9- or 12-column table: a fisheye row takes fisheye_ray, any other capture_ray unchanged (rsn_camera.h lens_ray)
__global__ __launch_bounds__(256) void rsn_capture_rays_image2_kernel(int height, int width, const float* c2w, const float* camera,
                                                                      int camera_stride, float* origins, float* directions,
                                                                      float* pixel_area) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= height * width) return;
  const int y = p / width, x = p - y * width;
  float o[3], d[3], area;
  lens_ray(c2w, load_lens_camera(camera, camera_stride), y, x, o, d, &area);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    origins[3 * p + j] = o[j];
    directions[3 * p + j] = d[j];
  }
  pixel_area[p] = area;
}

// ------------------------------------------------------------------------------------------------ depth targets
// The target distance along the normalised ray of every sampled pixel (include/rsn.h, "depth supervision"): one lane per ray, a
// 4-byte gather from the depth images and, for a z-depth, the length of the pixel centre's un-normalised camera-space direction
// v = (X, -Y, -1) in fp64 ((X, Y) from undistort_point for a distorted row).  A ray of a pyramid level above 0, a stored 0, an index
// outside the images and a fisheye row whose depth is not euclidean (no z-plane: the host refuses it) give 0, "no target".
struct GatherDepthArgs {
  int32_t n_rays, n_images, height, width;
  const int32_t* indices;  // [R, 3] = (image, y, x)
  const int32_t* level;    // [R] or NULL
  const float* depths;     // [N, H, W]
  const float* cameras;    // [N, stride] or NULL: the shared intrinsics k
  int32_t stride;
  Intrinsics k;
  int32_t euclidean;
  float* t;
};

__global__ __launch_bounds__(256) void rsn_gather_ray_depth_kernel(GatherDepthArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_rays) return;
  const int i = a.indices[3 * (size_t)r], y = a.indices[3 * (size_t)r + 1], x = a.indices[3 * (size_t)r + 2];
  float out = 0.0f;
  const bool level0 = !a.level || a.level[r] == 0;
  if (level0 && i >= 0 && i < a.n_images && y >= 0 && y < a.height && x >= 0 && x < a.width) {
    const float z = a.depths[((size_t)i * a.height + y) * a.width + x];
    if (a.euclidean) {
      out = z;
    } else if (z != 0.0f) {
      LensCamera lc{Camera{a.k, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, false};
      if (a.cameras) lc = load_lens_camera(a.cameras + (size_t)i * a.stride, a.stride);
      if (!lc.fisheye) {
        const Camera& c = lc.c;
        double X = ((double)x + 0.5 - (double)c.k.cx) / (double)c.k.fx, Y = ((double)y + 0.5 - (double)c.k.cy) / (double)c.k.fy;
        if (!(c.k1 == 0.0f && c.k2 == 0.0f && c.k3 == 0.0f && c.p1 == 0.0f && c.p2 == 0.0f)) undistort_point(c, X, Y, &X, &Y);
        out = (float)((double)z * sqrt(X * X + Y * Y + 1.0));
      }
    }
  }
  a.t[r] = out;
}

// ------------------------------------------------------------------------------------------------ SSIM
// One workgroup per SSIM_TX x SSIM_TY tile of window positions (position (py, px) = the 11 x 11 window whose top-left
// pixel is (py, px)).  Per channel: the (TY+10) x (TX+10) input patch of both images goes to LDS, a horizontal 11-tap pass
// writes the five moment rows (x, y, x^2, y^2, xy filtered) for TY+10 rows x TX columns to LDS, a vertical pass finishes
// the 2-D Gaussian per position and forms the SSIM term.  Moments never leave the workgroup; each workgroup writes one
// partial sum (fp64), and rsn_ssim_reduce_kernel adds the partials in a fixed order.
constexpr int SSIM_TX = 32, SSIM_TY = 16, SSIM_K = 11, SSIM_THREADS = 256;
constexpr int SSIM_PX = SSIM_TX + SSIM_K - 1, SSIM_PY = SSIM_TY + SSIM_K - 1;

struct SsimArgs {
  int32_t height, width;
  const float* pred;
  const float* target;
  const float* data_range;
  float taps[SSIM_K];
  double* partial;
  float* out;
};

__global__ __launch_bounds__(SSIM_THREADS) void rsn_ssim_tile_kernel(SsimArgs a) {
  __shared__ float sx[SSIM_PY][SSIM_PX + 1], sy[SSIM_PY][SSIM_PX + 1];
  __shared__ float hm[5][SSIM_PY][SSIM_TX + 1];
  __shared__ double red[SSIM_THREADS / 64];
  const int tid = threadIdx.x;
  const int ny = a.height - (SSIM_K - 1), nx = a.width - (SSIM_K - 1);  // window positions
  const int y0 = blockIdx.y * SSIM_TY, x0 = blockIdx.x * SSIM_TX;
  const float L = *a.data_range;
  const float c1 = (0.01f * L) * (0.01f * L), c2 = (0.03f * L) * (0.03f * L);
  float acc = 0.0f;
  for (int c = 0; c < 3; ++c) {
    __syncthreads();  // the previous channel's vertical pass is done with hm
    for (int e = tid; e < SSIM_PY * SSIM_PX; e += SSIM_THREADS) {
      const int ly = e / SSIM_PX, lx = e - ly * SSIM_PX;
      const int gy = y0 + ly, gx = x0 + lx;
      float vx = 0.0f, vy = 0.0f;
      if (gy < a.height && gx < a.width) {
        const size_t off = ((size_t)gy * a.width + gx) * 3 + c;
        vx = a.pred[off];
        vy = a.target[off];
      }
      sx[ly][lx] = vx;
      sy[ly][lx] = vy;
    }
    __syncthreads();
    for (int e = tid; e < SSIM_PY * SSIM_TX; e += SSIM_THREADS) {
      const int ly = e / SSIM_TX, lx = e - ly * SSIM_TX;
      float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < SSIM_K; ++t) {
        const float w = a.taps[t], p = sx[ly][lx + t], q = sy[ly][lx + t];
        m[0] += w * p;
        m[1] += w * q;
        m[2] += w * (p * p);
        m[3] += w * (q * q);
        m[4] += w * (p * q);
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) hm[j][ly][lx] = m[j];
    }
    __syncthreads();
    for (int e = tid; e < SSIM_TY * SSIM_TX; e += SSIM_THREADS) {
      const int ly = e / SSIM_TX, lx = e - ly * SSIM_TX;
      if (y0 + ly >= ny || x0 + lx >= nx) continue;
      float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < SSIM_K; ++t) {
        const float w = a.taps[t];
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] += w * hm[j][ly + t][lx];
      }
      const float mu_pp = m[0] * m[0], mu_tt = m[1] * m[1], mu_pt = m[0] * m[1];
      const float s_pp = m[2] - mu_pp, s_tt = m[3] - mu_tt, s_pt = m[4] - mu_pt;
      const float upper = 2.0f * s_pt + c2, lower = (s_pp + s_tt) + c2;
      acc += ((2.0f * mu_pt + c1) * upper) / ((mu_pp + mu_tt + c1) * lower);
    }
  }
  // fixed-order workgroup sum: butterfly within each wave, then the waves in order
  double s = acc;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < SSIM_THREADS / 64; ++w) t += red[w];
    a.partial[blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void rsn_ssim_reduce_kernel(const double* partial, int n_partial, double inv_count,
                                                              float* out) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n_partial; i += 256) s += partial[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) out[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) * inv_count);
}

inline dim3 ssim_grid(int height, int width) {
  return dim3((unsigned)((width - (SSIM_K - 1) + SSIM_TX - 1) / SSIM_TX),
              (unsigned)((height - (SSIM_K - 1) + SSIM_TY - 1) / SSIM_TY));
}

}  // namespace

extern "C" int rsn_sample_camera_rays(int32_t n_images, int32_t height, int32_t width, const uint8_t* images,
                                      const float* c2w, float fx, float fy, float cx, float cy, int32_t n_rays,
                                      uint32_t seed, uint32_t rank, uint32_t step, float* origins, float* directions,
                                      float* pixel_area, float* rgb, int32_t* indices, void* stream) {
  RSN_REQUIRE(n_images >= 1 && height >= 1 && width >= 1 && n_rays >= 0, RSN_ERR_INVALID_ARGUMENT,
              "n_images=%d height=%d width=%d n_rays=%d", n_images, height, width, n_rays);
  RSN_REQUIRE((uint64_t)n_images * (uint64_t)height * (uint64_t)width < (1ull << 32), RSN_ERR_INVALID_ARGUMENT,
              "n_images*height*width = %llu pixels: at most 2^32 - 1",
              (unsigned long long)n_images * height * width);
  RSN_REQUIRE(fx != 0.0f && fy != 0.0f, RSN_ERR_INVALID_ARGUMENT, "fx=%g fy=%g", (double)fx, (double)fy);
  if (n_rays == 0) return RSN_OK;
  RSN_REQUIRE(images && c2w && origins && directions && pixel_area && rgb && indices, RSN_ERR_INVALID_ARGUMENT,
              "a pointer is NULL");
  RSN_REQUIRE(((uintptr_t)images & 3) == 0, RSN_ERR_INVALID_ARGUMENT, "images must be 4-byte aligned");
  SampleArgs a{n_images, height, width, n_rays, images, c2w, Intrinsics{fx, fy, cx, cy}, seed, rank, step,
               origins, directions, pixel_area, rgb, indices};
  hipLaunchKernelGGL(rsn_sample_camera_rays_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_camera_rays_image(int32_t height, int32_t width, const float* c2w, float fx, float fy, float cx,
                                     float cy, float* origins, float* directions, float* pixel_area, void* stream) {
  RSN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= 0x7fffffff, RSN_ERR_INVALID_ARGUMENT,
              "height=%d width=%d", height, width);
  RSN_REQUIRE(fx != 0.0f && fy != 0.0f, RSN_ERR_INVALID_ARGUMENT, "fx=%g fy=%g", (double)fx, (double)fy);
  RSN_REQUIRE(c2w && origins && directions && pixel_area, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  const int n = height * width;
  hipLaunchKernelGGL(rsn_camera_rays_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     height, width, c2w, Intrinsics{fx, fy, cx, cy}, origins, directions, pixel_area);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_capture_rays_image(int32_t height, int32_t width, const float* c2w, const float* camera, float* origins,
                                      float* directions, float* pixel_area, void* stream) {
  RSN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= 0x7fffffff, RSN_ERR_INVALID_ARGUMENT,
              "height=%d width=%d", height, width);
  RSN_REQUIRE(c2w && camera && origins && directions && pixel_area, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  const int n = height * width;
  hipLaunchKernelGGL(rsn_capture_rays_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     height, width, c2w, camera, origins, directions, pixel_area);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_capture_rays_image2(int32_t height, int32_t width, const float* c2w, const float* camera, int32_t camera_stride,
                                       float* origins, float* directions, float* pixel_area, void* stream) {
  RSN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= 0x7fffffff, RSN_ERR_INVALID_ARGUMENT,
              "height=%d width=%d", height, width);
  RSN_REQUIRE(camera_stride == 9 || camera_stride == 12, RSN_ERR_INVALID_ARGUMENT, "camera_stride=%d: 9 or 12", camera_stride);
  RSN_REQUIRE(c2w && camera && origins && directions && pixel_area, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  const int n = height * width;
  hipLaunchKernelGGL(rsn_capture_rays_image2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     height, width, c2w, camera, camera_stride, origins, directions, pixel_area);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_gather_ray_depth(int32_t n_rays, const int32_t* indices, const int32_t* level, const float* depths,
                                    int32_t n_images, int32_t height, int32_t width, const float* cameras, int32_t camera_stride,
                                    float fx, float fy, float cx, float cy, int32_t has_fisheye, int32_t euclidean, float* t,
                                    void* stream) {
  RSN_REQUIRE(n_images >= 1 && height >= 1 && width >= 1 && n_rays >= 0, RSN_ERR_INVALID_ARGUMENT,
              "gather_ray_depth: n_images=%d height=%d width=%d n_rays=%d", n_images, height, width, n_rays);
  if (cameras) {
    RSN_REQUIRE(camera_stride == 9 || camera_stride == 12, RSN_ERR_INVALID_ARGUMENT, "gather_ray_depth: camera_stride=%d: 9 or 12",
                camera_stride);
    RSN_REQUIRE(!(has_fisheye && camera_stride != 12), RSN_ERR_INVALID_ARGUMENT,
                "gather_ray_depth: has_fisheye with a %d-column table (a fisheye row has 12 columns)", camera_stride);
  } else {
    RSN_REQUIRE(fx != 0.0f && fy != 0.0f, RSN_ERR_INVALID_ARGUMENT, "gather_ray_depth: fx=%g fy=%g", (double)fx, (double)fy);
    RSN_REQUIRE(!has_fisheye, RSN_ERR_INVALID_ARGUMENT, "gather_ray_depth: has_fisheye without a camera table");
  }
  RSN_REQUIRE(!(has_fisheye && !euclidean), RSN_ERR_INVALID_ARGUMENT,
              "gather_ray_depth: a fisheye row has no z-plane beyond 90 degrees: its depth files must hold distances along the ray "
              "(euclidean != 0)");
  if (n_rays == 0) return RSN_OK;
  RSN_REQUIRE(indices && depths && t, RSN_ERR_INVALID_ARGUMENT, "gather_ray_depth: indices, depths or t is NULL");
  const GatherDepthArgs a{n_rays, n_images, height, width, indices, level, depths, cameras, camera_stride,
                          Intrinsics{fx, fy, cx, cy}, euclidean != 0 ? 1 : 0, t};
  hipLaunchKernelGGL(rsn_gather_ray_depth_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" size_t rsn_ssim_workspace_bytes(int32_t height, int32_t width) {
  if (height < SSIM_K || width < SSIM_K) return 0;
  const dim3 g = ssim_grid(height, width);
  return (size_t)g.x * g.y * sizeof(double);
}

extern "C" int rsn_ssim(int32_t height, int32_t width, const float* pred, const float* target, const float* data_range,
                        void* workspace, size_t workspace_bytes, float* out, void* stream) {
  RSN_REQUIRE(height >= SSIM_K && width >= SSIM_K, RSN_ERR_INVALID_ARGUMENT,
              "SSIM needs images of at least %d x %d pixels (the Gaussian window), got %d x %d", SSIM_K, SSIM_K, height,
              width);
  RSN_REQUIRE((int64_t)height * width * 3 <= ((int64_t)1 << 40), RSN_ERR_INVALID_ARGUMENT, "height=%d width=%d", height,
              width);
  RSN_REQUIRE(pred && target && data_range && workspace && out, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  const size_t need = rsn_ssim_workspace_bytes(height, width);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  RSN_REQUIRE(((uintptr_t)workspace & 7) == 0, RSN_ERR_INVALID_ARGUMENT, "workspace must be 8-byte aligned");
  SsimArgs a{height, width, pred, target, data_range, {}, (double*)workspace, out};
  // torchmetrics _gaussian: exp(-(k / sigma)^2 / 2), k = -5..5, sigma = 1.5, normalised (in fp32, as torch computes it)
  float sum = 0.0f;
  for (int t = 0; t < SSIM_K; ++t) {
    const float k = (float)(t - SSIM_K / 2) / 1.5f;
    a.taps[t] = expf(-(k * k) / 2.0f);
  }
  for (int t = 0; t < SSIM_K; ++t) sum += a.taps[t];
  for (int t = 0; t < SSIM_K; ++t) a.taps[t] /= sum;
  const dim3 g = ssim_grid(height, width);
  hipLaunchKernelGGL(rsn_ssim_tile_kernel, g, dim3(SSIM_THREADS), 0, (hipStream_t)stream, a);
  const double count = 3.0 * (double)(height - (SSIM_K - 1)) * (double)(width - (SSIM_K - 1));
  hipLaunchKernelGGL(rsn_ssim_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                     (int)(g.x * g.y), 1.0 / count, out);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
