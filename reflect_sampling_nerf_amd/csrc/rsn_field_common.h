// rsn_field_common.h -- what ALL field kernel families share: the argument blocks, the tile space of a multi-job launch, and the
// reference's per-sample forward maths around the GEMMs (point -> contracted Gaussian, the head outputs, the colour combine),
// stated once as row / point functions.  Users: rsn_field_kernel.h (exact fp32 / split-bf16 / per-wave training),
// rsn_field_bf16.hip (plain-bf16 eval), rsn_field_bf16_train.hip and rsn_field_x6_train.hip (LDS-ring training).  The
// backward counterpart is rsn_field_bwd_common.h.  What stays per family: the GEMM loops, the operand formats, the encode loops
// (the per-wave family's loops and epilogues: rsn_gemm_loops.h, rsn_epilogues.h).  The scalar maths below builds on is
// rsn_device_math.h, the one header this one needs.
#pragma once
#include "rsn_device_math.h"

// What every evaluation of one launch shares (the network) ...
struct FieldShared {
  const float* packed;
  RsnPackedLayout L;
  int num_layers, skip_layer, width;
  float density_bias;
  float freqs[RSN_NUM_FREQS];
};

// ... and what one evaluation ("job") brings: its points, inputs and outputs.
struct FieldJob {
  int mode;
  int n_rays;          // rays (frustum / inf) or points (gauss)
  const int* n_dev;    // optional device-side ray count
  int S;               // samples per ray (1 for inf / gauss)
  const float* origins;
  const float* directions;
  const float* pixel_area;
  const float* bins;
  const float* sqradius;
  const float* means;
  const float* cov_diag;
  const float* view_dirs;
  rsn_field_outputs out;
  float* embedding;
  const float* emb_in;        // RSN_MODE_EMB: [N,W] embedding (post-ReLU trunk output) supplied by the caller
  const float* rough_in;      // RSN_MODE_EMB: optional explicit roughness for the SH attenuation (get_mid's argument)
  rsn_field_saved saved;      // training: activations kept for the backward pass (all NULL in eval)
  long long act_stride;       // floats between consecutive layers in saved.act (= n_points_max * W)
};

// one evaluation per launch (the plain-bf16 eval kernels of rsn_field_bf16.hip)
struct FieldArgs : FieldShared, FieldJob {};

// Several evaluations in ONE launch of rsn_field_kernel: the tiles of job 0, then job 1, ... form one tile space that
// the persistent workgroups stride through.  The reflect branch of a training step has three evaluations of a few
// hundred to ~1,250 tiles each on 256 workgroups; launched one by one, each wastes its last partial round of tiles
// (0.3-0.5 ms a round) and get_inf_color's ~20 tiles occupy 20 CUs for a whole launch.
#define RSN_MAX_JOBS 3
struct FieldJobs {
  FieldShared s;
  int n_jobs;
  FieldJob j[RSN_MAX_JOBS];
};

// The tile space of a multi-job launch: job k owns tiles [tb_k, tb_k+1) of TILE points (its ray count may live on the device).
struct TileJobs {
  long long np0, np1, np2, tb1, tb2, n_tiles;
};
template <int TILE = 256, class JOBS>
__device__ __forceinline__ TileJobs tile_space(const JOBS& J) {
  TileJobs t = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < RSN_MAX_JOBS; ++k) {
    if (k < J.n_jobs) {
      int nr = J.j[k].n_rays;
      if (J.j[k].n_dev) {
        const int nd = *J.j[k].n_dev;
        nr = nd < nr ? nd : nr;
      }
      const long long np = (long long)nr * J.j[k].S;
      if (k == 0) t.np0 = np; else if (k == 1) t.np1 = np; else t.np2 = np;
      t.n_tiles += (np + TILE - 1) / TILE;
    }
    if (k == 0) t.tb1 = t.n_tiles; else if (k == 1) t.tb2 = t.n_tiles;
  }
  return t;
}
// tile `gtile` of that space: whose it is, how many points that job has, which of the job's tiles (all workgroup-uniform)
struct TileAt {
  int job;
  long long n_points, tile;
};
__device__ __forceinline__ TileAt tile_at(const TileJobs& T, long long gtile) {
  const int jk = (gtile >= T.tb1 ? 1 : 0) + (gtile >= T.tb2 ? 1 : 0);
  return {jk, jk == 0 ? T.np0 : (jk == 1 ? T.np1 : T.np2), gtile - (jk == 0 ? 0 : (jk == 1 ? T.tb1 : T.tb2))};
}

// Conical frustum -> Gaussian (nerfstudio conical_frustum_to_gaussian / compute_3d_gaussian, N3),
// followed by the reference's contraction (reflect_sampling_nerf_field.py:98-119).  Only the diagonal
// of J Sigma J is consumed downstream (N2), so only that is formed.
__device__ __forceinline__ void frustum_to_contracted(const float o[3], const float d[3], float pa, float t0, float t1,
                                                      float mean_c[3], float var_c[3]) {
  const float radius = sqrtf(pa) / 1.7724538509055159f;
  const float mu = (t0 + t1) / 2.0f;
  const float hw = (t1 - t0) / 2.0f;
  const float hw2 = hw * hw, mu2 = mu * mu;
  const float den = 3.0f * mu2 + hw2;
  const float tmean = mu + (2.0f * mu * hw2) / den;
  float mean[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) mean[c] = o[c] + d[c] * tmean;
  const float hw4 = hw2 * hw2;
  const float var_t = hw2 / 3.0f - 0.26666666666666666f * ((hw4 * (12.0f * mu2 - hw2)) / (den * den));
  const float var_r =
      (radius * radius) * (mu2 / 4.0f + 0.4166666666666667f * hw2 - (0.26666666666666666f * hw4) / den);
  const float dmag = fmaxf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], 1e-10f);
  // Sigma = var_t d d^T + var_r (I - d (d/dmag)^T)
  float S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      S[i][j] = var_t * (d[i] * d[j]) + var_r * ((i == j ? 1.0f : 0.0f) - d[i] * (d[j] / dmag));
  // contraction
  const float n2 = mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2];
  const float n = sqrtf(n2);
  if (n > 1.0f) {
    const float sc = (2.0f * n - 1.0f) / n2;
    float J[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float eye = (i == j) ? 1.0f : 0.0f;
        const float outer = mean[i] * mean[j] / n2;
        J[i][j] = ((2.0f * n - 2.0f) * (eye - outer) + eye) / n2;
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) mean_c[c] = sc * mean[c];
    // diag(J S J)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const float js = J[i][0] * S[0][b] + J[i][1] * S[1][b] + J[i][2] * S[2][b];
        acc += js * J[b][i];
      }
      var_c[i] = fmaxf(acc, 0.0f);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mean_c[c] = mean[c];
      var_c[c] = fmaxf(S[c][c], 0.0f);
    }
  }
}


// ------------------------------------------------------------------------------------------------ per-sample maths
// The reference's per-sample formulas around the GEMMs, stated ONCE for every kernel family (their backward: rsn_field_bwd_common.h).
// The families differ in lane layout, so these take a point index and a heads ROW, not a lane: the heads are four rows of four
// values -- row 0 = (raw density, normal head x 3), row 1 = diff, row 2 = (raw roughness), row 3 = tint.  On the ring kernels lane
// group g owns row g; on the per-wave kernels half h owns rows h and h + 2.

// bf16-mode activations: sigmoid / softplus on v_exp_f32 / v_log_f32 / v_rcp_f32 (~1e-6 relative) instead of the
// correctly-rounded library forms -- their results are weighed against bf16 GEMM rounding (2^-9) in this mode
__device__ __forceinline__ float fast_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_softplus(float x) {
  return x > 20.0f ? x : 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(1.4426950408889634f * x));
}
// The arithmetic flavour of a kernel family: FAST = the plain-bf16 kernels on the LDS ring, else the correctly-rounded forms.
template <bool FAST>
struct FieldMath {
  static __device__ __forceinline__ float sigmoid(float x) { return FAST ? fast_sigmoid(x) : sigmoid_f(x); }
  static __device__ __forceinline__ float softplus(float x) { return FAST ? fast_softplus(x) : softplus_f(x); }
};

// Point pc of a FRUSTUM / INF job -> its contracted Gaussian (mean mc, diagonal variance vc) and view direction vd; returns
// whether the SH inputs see the direction.  IDX: the caller's index type (32-bit where the launcher bounds the point count).
template <class IDX>
__device__ __forceinline__ bool point_gaussian(const FieldJob& a, IDX pc, float (&mc)[3], float (&vc)[3], float (&vd)[3]) {
  if (a.mode == RSN_MODE_FRUSTUM) {
    const IDX rayi = pc / (IDX)a.S;
    const int s = (int)(pc - rayi * (IDX)a.S);
    const size_t ray = (size_t)rayi;
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = a.origins[ray * 3 + c];
      vd[c] = a.directions[ray * 3 + c];
    }
    frustum_to_contracted(o, vd, a.pixel_area[ray], a.bins[ray * (a.S + 1) + s], a.bins[ray * (a.S + 1) + s + 1], mc, vc);
    return true;
  }
  // RSN_MODE_INF (reflect_sampling_nerf_field.py:190-199)
  const float r2 = a.sqradius[pc];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    vd[c] = a.directions[(size_t)pc * 3 + c];
    mc[c] = 2.0f * vd[c];
    vc[c] = (0.6f * r2) * (1.0f - vd[c] * vd[c]);
  }
  return false;  // SH inputs are zeroed (reflect_sampling_nerf_field.py:199)
}

// get_pred_normals: -normalize(head), then normalize again (field.py:139-144, N6)
__device__ __forceinline__ void pred_normal(float r1, float r2, float r3, float (&n)[3]) {
  float nrm = fmaxf(sqrtf(r1 * r1 + r2 * r2 + r3 * r3), 1e-12f);
  float nx = -(r1 / nrm), ny = -(r2 / nrm), nz = -(r3 / nrm);
  nrm = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-12f);
  n[0] = nx / nrm; n[1] = ny / nrm; n[2] = nz / nrm;
}

// Outputs of heads row `row` of VALID point q: r = the row's pre-activations, col = sigmoid of r.x .. r.z (the caller keeps
// them for the colour combine).  SAVE: also the row's share of saved.heads (raw normal head, raw roughness), kept for every mode.
template <bool FAST, bool SAVE, class IDX>
__device__ __forceinline__ void head_outputs_row(int row, const FieldJob& a, float density_bias, IDX q, float4 r,
                                                 const float (&col)[3], const float (&vd)[3]) {
  const bool out = a.mode != RSN_MODE_INF;
  if (row == 0) {
    if (SAVE && a.saved.heads) { a.saved.heads[q * 8 + 0] = r.y; a.saved.heads[q * 8 + 1] = r.z; a.saved.heads[q * 8 + 2] = r.w; }
    if (out) {
      float n[3];
      pred_normal(r.y, r.z, r.w, n);
      if (a.out.sigma) a.out.sigma[q] = FieldMath<FAST>::softplus(r.x + density_bias);
      if (a.out.raw_density) a.out.raw_density[q] = r.x;
      if (a.out.pred_normals) {
        a.out.pred_normals[q * 3 + 0] = n[0];
        a.out.pred_normals[q * 3 + 1] = n[1];
        a.out.pred_normals[q * 3 + 2] = n[2];
      }
      if (a.out.n_dot_d) a.out.n_dot_d[q] = vd[0] * n[0] + vd[1] * n[1] + vd[2] * n[2];
    }
  } else if (row == 2) {
    if (SAVE && a.saved.heads) a.saved.heads[q * 8 + 3] = r.x;
    if (out) {
      if (a.out.roughness) a.out.roughness[q] = col[0];
      if (a.out.raw_roughness) a.out.raw_roughness[q] = r.x;
    }
  } else {
    float* dst = row == 1 ? a.out.diff : a.out.tint;
    if (out && dst) { dst[q * 3 + 0] = col[0]; dst[q * 3 + 1] = col[1]; dst[q * 3 + 2] = col[2]; }
  }
}

// Colour of VALID point q from the RGB head's pre-activations z: diff + tint * mid (INF, or heads-only calls that ask for
// neither diff nor tint: mid alone).  SAVE: mid is kept in saved.heads + 4.
template <bool FAST, bool SAVE, class IDX>
__device__ __forceinline__ void colour_out(const FieldJob& a, IDX q, float z0, float z1, float z2, const float (&dif)[3],
                                           const float (&tin)[3]) {
  const float m0 = FieldMath<FAST>::sigmoid(z0), m1 = FieldMath<FAST>::sigmoid(z1), m2 = FieldMath<FAST>::sigmoid(z2);
  if (SAVE && a.saved.heads) *reinterpret_cast<float4*>(a.saved.heads + q * 8 + 4) = make_float4(m0, m1, m2, 0.0f);
  if (a.out.color) {
    if (a.mode == RSN_MODE_INF || (a.mode == RSN_MODE_EMB && !a.out.diff && !a.out.tint)) {
      a.out.color[q * 3 + 0] = m0; a.out.color[q * 3 + 1] = m1; a.out.color[q * 3 + 2] = m2;
    } else {
      a.out.color[q * 3 + 0] = dif[0] + tin[0] * m0;
      a.out.color[q * 3 + 1] = dif[1] + tin[1] * m1;
      a.out.color[q * 3 + 2] = dif[2] + tin[2] * m2;
    }
  }
}


// ------------------------------------------------------------------------------------------------ host side: filling a launch
// Shared by the forward (rsn_field.hip) and backward (rsn_field_bwd.hip) entry points, whose blocks name what they have in common
// alike.  A single call is a one-job launch: `pfx` is "" there and JobPrefix(k).s = "job k: " for evaluation k of a *_jobs call.
struct JobPrefix {
  char s[16];
  explicit JobPrefix(int k) { snprintf(s, sizeof(s), "job %d: ", k); }
};

// The network of a launch (FieldShared / BwdShared): its packed layout and the descriptor's constants.
template <class SHARED>
inline int rsn_fill_shared(SHARED& s, const rsn_field_desc* d, const float* packed) {
  RSN_TRY(rsn_compute_layout(d, &s.L));
  RSN_REQUIRE(packed != nullptr, RSN_ERR_INVALID_ARGUMENT, "packed weights pointer is NULL");
  s.packed = packed;
  s.num_layers = d->num_layers;
  s.skip_layer = d->skip_layer;
  s.density_bias = d->density_bias;
  for (int i = 0; i < RSN_NUM_FREQS; ++i) s.freqs[i] = d->freqs[i];
  return RSN_OK;
}

// Tiles of `tile` points over the jobs of a launch, by the host-side ray counts (an upper bound of what the device counts give).
template <class JOBS>
inline long long rsn_job_tiles(const JOBS& J, int tile) {
  long long n = 0;
  for (int k = 0; k < J.n_jobs; ++k) n += ((long long)J.j[k].n_rays * J.j[k].S + tile - 1) / tile;
  return n;
}

// The fillers of the two kinds both directions have (FieldJob / BwdJob): check the kind's input pointers, set its fields.  The
// counts are checked by the entry points, whose wording differs.  INF's rgb: its colour (forward) / that colour's gradient.
template <class JOB>
inline int rsn_fill_frustum(JOB& a, const char* pfx, int n_rays, const int* n_dev, int n_samples, const float* origins,
                            const float* directions, const float* pixel_area, const float* euclid_bins) {
  RSN_REQUIRE(n_rays == 0 || (origins && directions && pixel_area && euclid_bins), RSN_ERR_INVALID_ARGUMENT,
              "%sa ray input pointer is NULL", pfx);
  a.mode = RSN_MODE_FRUSTUM;
  a.n_rays = n_rays; a.n_dev = n_dev; a.S = n_samples;
  a.origins = origins; a.directions = directions; a.pixel_area = pixel_area; a.bins = euclid_bins;
  return RSN_OK;
}
template <class JOB>
inline int rsn_fill_inf(JOB& a, const char* pfx, int n_rays, const int* n_dev, const float* directions, const float* sqradius,
                        const float* rgb) {
  RSN_REQUIRE(n_rays == 0 || (directions && sqradius && rgb), RSN_ERR_INVALID_ARGUMENT, "%san input pointer is NULL", pfx);
  a.mode = RSN_MODE_INF;
  a.n_rays = n_rays; a.n_dev = n_dev; a.S = 1;
  a.directions = directions; a.sqradius = sqradius;
  return RSN_OK;
}

// The per-wave kernels (rsn_field_kernel, rsn_field_bwd_kernel) are built for three widths: `launch` gets NB = width / 32 row
// blocks as a compile-time constant, std::integral_constant<int, NB>.
template <class LAUNCH>
inline int rsn_for_width(int width, LAUNCH&& launch) {
  switch (width) {
    case 256: launch(std::integral_constant<int, 8>()); break;
    case 128: launch(std::integral_constant<int, 4>()); break;
    case 64: launch(std::integral_constant<int, 2>()); break;
    default: RSN_REQUIRE(false, RSN_ERR_UNSUPPORTED, "width=%d unsupported", width);
  }
  return RSN_OK;
}

// rsn_field_bf16.hip: the dedicated RSN_MMA_BF16 eval kernel (two workgroups per CU)
int rsn_launch_field_bf16(int width, long long grid, hipStream_t st, const FieldArgs& a);
// split-bf16 instantiations of rsn_field_kernel (rsn_field_split.hip): RSN_MMA_BF16X6, or RSN_MMA_BF16X3 (eval only)
int rsn_launch_field_split(int width, bool train, rsn_mma_mode mode, long long grid, hipStream_t st, const FieldJobs& J);
