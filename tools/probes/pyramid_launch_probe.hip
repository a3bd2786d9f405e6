// pyramid_launch_probe.hip -- rsn_build_pyramid as ONE launch with a level table (the library's kernel, included below as it
// stands) against ONE LAUNCH PER LEVEL (the same lane body with the level as an argument), on N images of S x S RGBA noise.
// Both variants must write the same bytes; each is timed between two HIP events, alternating, after 3 untimed runs.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I include -I reflect_sampling_nerf_amd/csrc \
//         tools/probes/pyramid_launch_probe.hip -o tools/probes/pyramid_launch_probe
//   tools/probes/pyramid_launch_probe [N=100] [S=800] [L=4] [reps=20]      -> one JSON line
#include "../../reflect_sampling_nerf_amd/csrc/rsn_pyramid.hip"

#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>

void rsn_set_error(const char* fmt, ...) {  // the library's lives in rsn_pack.hip
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

namespace {

// level l alone: lane q owns pixel q of the level; the body is rsn_build_pyramid_kernel's
__global__ __launch_bounds__(256) void one_level_kernel(PyramidArgs a, int l) {
  const uint32_t wl = (uint32_t)(a.width >> l), hwl = (uint32_t)(a.height >> l) * wl;
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= hwl * (uint32_t)a.n_images) return;
  const uint32_t i = q / hwl, rem = q - i * hwl;
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
  const float den = (float)(65025u * (uint32_t)(s * s));
  const size_t p = (size_t)a.t.off[l] + q;
  for (int j = 0; j < 3; ++j) a.pyramid[p * 3 + j] = (float)S[j] / den;
}

#define CHECK(call)                                                                         \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "%s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      return 1;                                                                             \
    }                                                                                       \
  } while (0)

double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return 0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
}

}  // namespace

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 100, S = argc > 2 ? atoi(argv[2]) : 800, L = argc > 3 ? atoi(argv[3]) : 4;
  const int reps = argc > 4 ? atoi(argv[4]) : 20;
  if (check_pyramid_shape(N, S, S, L) != RSN_OK || L < 2 || reps < 1) return 2;
  const LevelTable t = level_table(N, S, S, L);
  const size_t n_px = (size_t)N * S * S, pyr_px = t.off[L];
  std::vector<uint32_t> host(n_px);
  uint32_t x = 12345u;
  for (auto& v : host) {  // RGBA noise
    x = x * 1664525u + 1013904223u;
    v = x ^ (x >> 13);
  }
  uint8_t* images = nullptr;
  float *one = nullptr, *per = nullptr;
  CHECK(hipMalloc(&images, n_px * 4));
  CHECK(hipMalloc(&one, pyr_px * 12));
  CHECK(hipMalloc(&per, pyr_px * 12));
  CHECK(hipMemcpy(images, host.data(), n_px * 4, hipMemcpyHostToDevice));
  CHECK(hipMemset(one, 0xff, pyr_px * 12));
  CHECK(hipMemset(per, 0xee, pyr_px * 12));
  auto run_one = [&]() { return rsn_build_pyramid(N, S, S, L, images, one, pyr_px, nullptr); };
  auto run_per = [&]() {
    const PyramidArgs a{N, S, S, L, images, per, t};
    for (int l = 1; l < L; ++l) {
      const uint32_t n = (uint32_t)N * (uint32_t)(S >> l) * (uint32_t)(S >> l);
      hipLaunchKernelGGL(one_level_kernel, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, a, l);
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
  };
  for (int w = 0; w < 3; ++w)
    if (run_one() != 0 || run_per() != 0) return 1;
  CHECK(hipDeviceSynchronize());
  std::vector<float> a(pyr_px * 3), b(pyr_px * 3);
  CHECK(hipMemcpy(a.data(), one, pyr_px * 12, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(b.data(), per, pyr_px * 12, hipMemcpyDeviceToHost));
  const bool same = memcmp(a.data(), b.data(), pyr_px * 12) == 0;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> t_one, t_per;
  for (int r = 0; r < reps; ++r)
    for (int v = 0; v < 2; ++v) {
      float ms = 0.0f;
      CHECK(hipEventRecord(e0, nullptr));
      if ((v == 0 ? run_one() : run_per()) != 0) return 1;
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      (v == 0 ? t_one : t_per).push_back(ms);
    }
  printf("{\"images\": %d, \"size\": %d, \"levels\": %d, \"reps\": %d, \"same_bytes\": %s, \"one_launch_ms\": {\"median\": %.4f, \"min\": %.4f}, "
         "\"launch_per_level_ms\": {\"median\": %.4f, \"min\": %.4f}}\n",
         N, S, L, reps, same ? "true" : "false", median(t_one), *std::min_element(t_one.begin(), t_one.end()), median(t_per),
         *std::min_element(t_per.begin(), t_per.end()));
  return same ? 0 : 3;
}
