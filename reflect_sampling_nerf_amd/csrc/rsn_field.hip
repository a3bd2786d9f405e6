// rsn_field.hip -- the dominant kernel: fused per-sample field evaluation on gfx950.
//
// One wavefront owns a tile of 32 sample points for the whole network.  With
// v_mfma_f32_32x32x2_f32 computing D[n][m] = sum_k W[n][k] * X[m][k] (A = weights, B = points) the
// accumulator of lane (m = lane&31, h = lane>>5) holds, for ITS point m, output features
// nb*32 + 8q + 4h + j (register 4q+j).  The K index of the next layer is a free permutation, and the
// packed weights (rsn_pack.hip) are laid out so that K-iteration `it` (8 features) consumes from
// lane (m,h) exactly features it*8 + 4h + {0..3}: the four registers that lane already holds.
// So activations never cross lanes between layers: each lane parks its float4's in a wave-private
// LDS slab X[it][lane] (ds_write_b128 / ds_read_b128, conflict-free, no barriers) purely so that the
// K loop can index them dynamically.  Weights stream L2 -> VGPR as 1 KiB-contiguous
// global_load_dwordx4 per (it, nb), double-buffered one K-iteration (2048 MFMA cycles) ahead.
//
// Roofline: MFMA-bound.  1,230,592 algorithmic FLOP per sample at W=256, L=8;
// the padded instruction stream issues 9,808 MFMAs per 32-point tile vs 9,614 algorithmic.
//
// Reference semantics restated here: reflect_sampling_nerf_field.py:90-207,
// reflect_sampling_nerf_components.py:52-140 and the nerfstudio primitives N1-N3, N6.
#include "rsn_field_kernel.h"
#include "rsn_field_bwd_common.h"

// ------------------------------------------------------------------------------------------------
// One launch over n evaluations of one field (all training or all eval; the plain-bf16 eval kernels take one).
static int launch_field_jobs(const rsn_field_desc* d, const float* packed, FieldJob* js, int n, void* stream) {
  RSN_REQUIRE(n >= 1 && n <= RSN_MAX_JOBS, RSN_ERR_INVALID_ARGUMENT, "n_jobs=%d (1..%d)", n, RSN_MAX_JOBS);
  FieldJobs J = {};
  RSN_TRY(rsn_fill_shared(J.s, d, packed));
  J.s.width = d->width;
  auto training = [](const FieldJob& a) { return a.saved.act != nullptr || a.saved.enc != nullptr || a.saved.heads != nullptr; };
  const bool train = training(js[0]);
  for (int k = 0; k < n; ++k) {
    FieldJob& a = js[k];
    if (a.n_rays <= 0) continue;
    RSN_REQUIRE(training(a) == train, RSN_ERR_INVALID_ARGUMENT, "job %d: training and eval evaluations cannot share a launch", k);
    a.act_stride = (long long)a.n_rays * a.S * (long long)d->width;
    J.j[J.n_jobs++] = a;
  }
  if (J.n_jobs == 0) return RSN_OK;
  const long long n_tiles = rsn_job_tiles(J, 128);
  const int cus = rsn_device_cus();
  // one 4-wave workgroup per CU (one wave per SIMD, LDS slab 148 KiB at W=256): persistent tiles
  const long long grid = n_tiles < (long long)cus ? n_tiles : (long long)cus;
  hipStream_t st = (hipStream_t)stream;
  const int mode = d->mma_mode;
  if (!train && mode == RSN_MMA_BF16) {  // plain bf16 operands: its own kernel, two workgroups per CU
    RSN_REQUIRE(J.n_jobs == 1, RSN_ERR_UNSUPPORTED, "the plain-bf16 eval kernels take one evaluation per launch");
    FieldArgs one = {};
    static_cast<FieldShared&>(one) = J.s;
    static_cast<FieldJob&>(one) = J.j[0];
    const long long g2 = n_tiles < 2LL * cus ? n_tiles : 2LL * cus;
    return rsn_launch_field_bf16(d->width, g2, st, one);
  }
  if (train && rsn_ring_training(d))  // plain / split bf16 training at width 256: the LDS-ring kernels (256- / 128-point tiles)
    return mode == RSN_MMA_BF16X6 ? rsn_launch_field_x6_train(n_tiles, st, J) : rsn_launch_field_bf16_train(rsn_job_tiles(J, 256), st, J);
  if (mode == RSN_MMA_BF16X6 || (!train && mode == RSN_MMA_BF16X3)) {  // split-bf16 instantiations: rsn_field_split.hip
    RSN_TRY(rsn_launch_field_split(d->width, train, (rsn_mma_mode)mode, grid, st, J));
    RSN_HIP(hipGetLastError());
    return RSN_OK;
  }
  RSN_TRY(rsn_for_width(d->width, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    const dim3 g((unsigned)grid), b(256);
    if (train && mode == RSN_MMA_BF16)  // reduced-precision training: plain bf16 operands, fp32 accumulate
      hipLaunchKernelGGL((rsn_field_kernel<NB, true, RSN_MMA_BF16>), g, b, 0, st, J);
    else if (train && mode == RSN_MMA_F32_FOLDED)  // exact fp32, the bottleneck folded into mlp_mid
      hipLaunchKernelGGL((rsn_field_kernel<NB, true, RSN_MMA_F32_FOLDED>), g, b, 0, st, J);
    else if (train)  // BF16X3 is an eval-only opt-in: training falls back to exact fp32
      hipLaunchKernelGGL((rsn_field_kernel<NB, true, RSN_MMA_F32>), g, b, 0, st, J);
    else
      hipLaunchKernelGGL((rsn_field_kernel<NB, false, RSN_MMA_F32>), g, b, 0, st, J);
  }));
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

static int launch_field(const rsn_field_desc* d, const float* pk, FieldJob& a, void* st) { return launch_field_jobs(d, pk, &a, 1, st); }

// The entry points: NULL-check the struct pointers, fill a zeroed FieldJob with the kind's filler (frustum and inf, which the
// backward has too: rsn_field_common.h), launch.  A training evaluation adds `saved` and this requirement (get_inf_color
// has no analytic normals, so its wording leaves them out).
static int require_saved(const rsn_field_desc* d, const char* pfx, const rsn_field_saved* s, bool inf) {
  const bool bott = s->bott || d->mma_mode == RSN_MMA_F32_FOLDED;  // the folded kernels have no bottleneck row
  RSN_REQUIRE(s->act && s->enc && bott && s->sh && s->hid && s->heads && s->relu_bits, RSN_ERR_INVALID_ARGUMENT,
              "%straining needs every saved-activation buffer%s", pfx, inf ? "" : " (normals may be NULL)");
  return RSN_OK;
}

static int fill_gaussians(FieldJob& a, int n_points, const float* means, const float* cov_diag, const float* view_dirs,
                          const rsn_field_outputs* out, float* embedding) {
  RSN_REQUIRE(n_points >= 0, RSN_ERR_INVALID_ARGUMENT, "n_points=%d", n_points);
  RSN_REQUIRE(n_points == 0 || means, RSN_ERR_INVALID_ARGUMENT, "means is NULL");
  a.mode = RSN_MODE_GAUSS;
  a.n_rays = n_points; a.S = 1;
  a.means = means; a.cov_diag = cov_diag; a.view_dirs = view_dirs;
  a.out = *out;
  a.embedding = embedding;
  return RSN_OK;
}

// rsn_field_forward_train_jobs: several training-mode evaluations of the SAME field in one launch.
extern "C" int rsn_field_forward_train_jobs(const rsn_field_desc* desc, const float* packed, int32_t n_jobs,
                                            const rsn_field_job* jobs, void* stream) {
  RSN_REQUIRE(desc && jobs, RSN_ERR_INVALID_ARGUMENT, "desc/jobs is NULL");
  RSN_REQUIRE(n_jobs >= 1 && n_jobs <= RSN_MAX_JOBS, RSN_ERR_INVALID_ARGUMENT, "n_jobs=%d (1..%d)", n_jobs, RSN_MAX_JOBS);
  FieldJob js[RSN_MAX_JOBS] = {};
  for (int k = 0; k < n_jobs; ++k) {
    const rsn_field_job& q = jobs[k];
    FieldJob& a = js[k];
    const JobPrefix pfx(k);
    RSN_REQUIRE(q.kind == 0 || q.kind == 1, RSN_ERR_INVALID_ARGUMENT, "job %d: kind=%d", k, q.kind);
    RSN_REQUIRE(q.n_rays >= 0 && q.saved, RSN_ERR_INVALID_ARGUMENT, "job %d: n_rays=%d / saved is NULL", k, q.n_rays);
    RSN_TRY(require_saved(desc, pfx.s, q.saved, false));
    a.saved = *q.saved;
    if (q.kind == 0) {
      RSN_REQUIRE(q.n_samples >= 1 && q.out, RSN_ERR_INVALID_ARGUMENT, "job %d: n_samples=%d / out is NULL", k, q.n_samples);
      RSN_TRY(rsn_fill_frustum(a, pfx.s, q.n_rays, q.n_dev, q.n_samples, q.origins, q.directions, q.pixel_area, q.euclid_bins));
      a.out = *q.out;
    } else {
      RSN_TRY(rsn_fill_inf(a, pfx.s, q.n_rays, q.n_dev, q.directions, q.sqradius, q.out_rgb));
      a.out.color = q.out_rgb;
      a.saved.normals = nullptr;
    }
  }
  return launch_field_jobs(desc, packed, js, n_jobs, stream);
}

extern "C" int rsn_field_forward_gaussians_train(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                                 const float* means, const float* cov_diag, const float* view_dirs,
                                                 const rsn_field_outputs* out, float* embedding,
                                                 const rsn_field_saved* saved, void* stream) {
  RSN_REQUIRE(desc && out && saved, RSN_ERR_INVALID_ARGUMENT, "desc/out/saved is NULL");
  FieldJob a = {};
  RSN_TRY(fill_gaussians(a, n_points, means, cov_diag, view_dirs, out, embedding));
  RSN_REQUIRE(desc->mma_mode == RSN_MMA_F32 || desc->mma_mode == RSN_MMA_F32_FOLDED, RSN_ERR_UNSUPPORTED,
              "training-mode evaluation of explicit Gaussians runs on the exact-fp32 kernels only (mma_mode %d)", desc->mma_mode);
  RSN_TRY(require_saved(desc, "", saved, false));
  a.saved = *saved;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_frustum(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                         const int32_t* n_dev, int32_t n_samples, const float* origins,
                                         const float* directions, const float* pixel_area, const float* euclid_bins,
                                         const rsn_field_outputs* out, void* stream) {
  RSN_REQUIRE(desc && out, RSN_ERR_INVALID_ARGUMENT, "desc/out is NULL");
  RSN_REQUIRE(n_rays >= 0 && n_samples >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d n_samples=%d", n_rays, n_samples);
  FieldJob a = {};
  RSN_TRY(rsn_fill_frustum(a, "", n_rays, n_dev, n_samples, origins, directions, pixel_area, euclid_bins));
  a.out = *out;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_frustum_train(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                               const int32_t* n_dev, int32_t n_samples, const float* origins,
                                               const float* directions, const float* pixel_area,
                                               const float* euclid_bins, const rsn_field_outputs* out,
                                               const rsn_field_saved* saved, void* stream) {
  RSN_REQUIRE(desc && out && saved, RSN_ERR_INVALID_ARGUMENT, "desc/out/saved is NULL");
  RSN_REQUIRE(n_rays >= 0 && n_samples >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d n_samples=%d", n_rays, n_samples);
  FieldJob a = {};
  RSN_TRY(rsn_fill_frustum(a, "", n_rays, n_dev, n_samples, origins, directions, pixel_area, euclid_bins));
  RSN_TRY(require_saved(desc, "", saved, false));
  a.out = *out;
  a.saved = *saved;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_inf(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                     const int32_t* n_dev, const float* directions, const float* sqradius,
                                     float* out_rgb, void* stream) {
  RSN_REQUIRE(desc, RSN_ERR_INVALID_ARGUMENT, "desc is NULL");
  RSN_REQUIRE(n_rays >= 0, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  FieldJob a = {};
  RSN_TRY(rsn_fill_inf(a, "", n_rays, n_dev, directions, sqradius, out_rgb));
  a.out.color = out_rgb;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_inf_train(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                           const int32_t* n_dev, const float* directions, const float* sqradius,
                                           float* out_rgb, const rsn_field_saved* saved, void* stream) {
  RSN_REQUIRE(desc && saved, RSN_ERR_INVALID_ARGUMENT, "desc/saved is NULL");
  RSN_REQUIRE(n_rays >= 0, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  FieldJob a = {};
  RSN_TRY(rsn_fill_inf(a, "", n_rays, n_dev, directions, sqradius, out_rgb));
  RSN_TRY(require_saved(desc, "", saved, true));
  a.out.color = out_rgb;
  a.saved = *saved;
  a.saved.normals = nullptr;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_embedding(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                           const float* embedding, const float* view_dirs, const float* roughness,
                                           const rsn_field_outputs* out, void* stream) {
  RSN_REQUIRE(desc && out, RSN_ERR_INVALID_ARGUMENT, "desc/out is NULL");
  RSN_REQUIRE(n_points >= 0, RSN_ERR_INVALID_ARGUMENT, "n_points=%d", n_points);
  RSN_REQUIRE(n_points == 0 || embedding, RSN_ERR_INVALID_ARGUMENT, "embedding is NULL");
  FieldJob a = {};  // the one entry point of its kind: filled here
  a.mode = RSN_MODE_EMB;
  a.n_rays = n_points; a.S = 1;
  a.emb_in = embedding; a.view_dirs = view_dirs; a.rough_in = roughness;
  a.out = *out;
  return launch_field(desc, packed, a, stream);
}

extern "C" int rsn_field_forward_gaussians(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                           const float* means, const float* cov_diag, const float* view_dirs,
                                           const rsn_field_outputs* out, float* embedding, void* stream) {
  RSN_REQUIRE(desc && out, RSN_ERR_INVALID_ARGUMENT, "desc/out is NULL");
  FieldJob a = {};
  RSN_TRY(fill_gaussians(a, n_points, means, cov_diag, view_dirs, out, embedding));
  return launch_field(desc, packed, a, stream);
}
