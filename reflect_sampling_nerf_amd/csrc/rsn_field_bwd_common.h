// rsn_field_bwd_common.h -- argument blocks of the backward sweeps and the reference's per-sample autograd, restated ONCE:
// head_grad_inputs / head_grad_row (softplus', the double-normalise backward, n_dot_d, the fused per-ray normal losses, the
// sigmoid derivatives of diff / tint / roughness / RGB) and input_grad_of_dvar (variance gradient -> pixel_area / sqradius).
// Users: rsn_field_bwd.hip (per-wave weight stream: exact fp32, split-bf16, plain bf16 at widths 64 / 128),
// rsn_field_bf16_train.hip and rsn_field_x6_train.hip (plain / split bf16 at width 256 on the LDS weight ring).
#pragma once
#include "rsn_field_common.h"

struct BwdShared {
  const float* packed;
  RsnPackedLayout L;
  int num_layers, skip_layer;
  float density_bias;
  float freqs[RSN_NUM_FREQS];
};

struct BwdJob {
  int mode, n_rays, S, need_input_grad;
  const int* n_dev;
  const float* origins;
  const float* directions;
  const float* pixel_area;
  const float* bins;
  const float* sqradius;
  rsn_field_grads_in gin;
  rsn_field_outputs fwd;   // forward per-sample values: raw_density, diff, tint
  rsn_field_saved saved;
  rsn_field_grads_out gout;
  long long act_stride;
};

// Several evaluations in one launch (see FieldJobs, rsn_field_common.h): the backward sweeps of the two reflect levels and
// of get_inf_color are independent of each other once the compositing backward of both levels has run.
struct BwdJobs {
  BwdShared s;
  int n_jobs;
  BwdJob j[RSN_MAX_JOBS];
};

// d var_c / d pixel_area for a conical-frustum sample after contraction (the mean does not depend on pixel_area):
// var_c = relu(diag(J Sigma J))_c, Sigma = var_t d d^T + var_r (I - d (d/|d|^2)^T), var_r = (pa / 1.7724538509^2) Kr(t).
__device__ __forceinline__ void frustum_dvar_dpa(const float o[3], const float d[3], float pa, float t0, float t1,
                                                 float out[3]) {
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
  const float kr = mu2 / 4.0f + 0.4166666666666667f * hw2 - (0.26666666666666666f * hw4) / den;
  const float var_r = (radius * radius) * kr;
  const float dmag = fmaxf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], 1e-10f);
  float S[3][3], Nn[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Nn[i][j] = (i == j ? 1.0f : 0.0f) - d[i] * (d[j] / dmag);
      S[i][j] = var_t * (d[i] * d[j]) + var_r * Nn[i][j];
    }
  const float n2 = mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2];
  const float n = sqrtf(n2);
  float J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float eye = (i == j) ? 1.0f : 0.0f;
      J[i][j] = (n > 1.0f) ? ((2.0f * n - 2.0f) * (eye - mean[i] * mean[j] / n2) + eye) / n2 : eye;
    }
  // d(radius^2)/d(pa) = 1 / 1.7724538509^2
  const float dr2 = kr / (1.7724538509055159f * 1.7724538509055159f);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float vs = 0.0f, vn = 0.0f;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float js = J[i][0] * S[0][b] + J[i][1] * S[1][b] + J[i][2] * S[2][b];
      const float jn = J[i][0] * Nn[0][b] + J[i][1] * Nn[1][b] + J[i][2] * Nn[2][b];
      vs += js * J[b][i];
      vn += jn * J[b][i];
    }
    out[i] = vs > 0.0f ? vn * dr2 : 0.0f;  // relu on the diagonal (reflect_sampling_nerf_field.py:114-115)
  }
}

// F.normalize backward: y = x / max(|x|, eps);  g_x = (g_y - y (y . g_y)) / |x|
__device__ __forceinline__ void normalize_bwd(const float x[3], const float gy[3], float gx[3]) {
  const float len = fmaxf(sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), 1e-12f);
  const float y0 = x[0] / len, y1 = x[1] / len, y2 = x[2] / len;
  const float dot = y0 * gy[0] + y1 * gy[1] + y2 * gy[2];
  gx[0] = (gy[0] - y0 * dot) / len;
  gx[1] = (gy[1] - y1 * dot) / len;
  gx[2] = (gy[2] - y2 * dot) / len;
}


// ------------------------------------------------------------------------------------------------ the reference's autograd, per sample
// Restated ONCE for the three backward sweeps (reference: reflect_sampling_nerf_model.py:142-344, field.py:122-207; the summary
// is at the top of rsn_field_bwd.hip).  Like the forward pieces (rsn_field_common.h) these take a point index and a heads ROW.

// What every heads row of point q needs: the colour gradient, the forward values it is chained through, and the RGB head's
// pre-activation gradient dz (colour = diff + tint * mid, INF: colour = mid; mid = sigmoid(z)).  `live`: 0 on padded lanes.
struct HeadGradIn {
  float gcol[3], mid[3], dif[3], tin[3], dz[3];
  float4 hd;  // saved raw normal head (3), raw roughness
};
template <class IDX>
__device__ __forceinline__ void head_grad_inputs(const BwdJob& a, IDX q, float live, bool store_dz, HeadGradIn& v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) v.gcol[c] = 0.0f;
  if (a.gin.color) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v.gcol[c] = a.gin.color[q * 3 + c] * live;
  }
  v.hd = *reinterpret_cast<const float4*>(a.saved.heads + q * 8);
  const float4 md = *reinterpret_cast<const float4*>(a.saved.heads + q * 8 + 4);   // mid RGB (3)
  v.mid[0] = md.x; v.mid[1] = md.y; v.mid[2] = md.z;
#pragma unroll
  for (int c = 0; c < 3; ++c) { v.dif[c] = 0.0f; v.tin[c] = 1.0f; }
  if (a.mode != RSN_MODE_INF) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v.dif[c] = a.fwd.diff[q * 3 + c];
      v.tin[c] = a.fwd.tint[q * 3 + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v.dz[c] = v.gcol[c] * v.tin[c] * (v.mid[c] * (1.0f - v.mid[c]));
  if (store_dz && a.gout.dz_rgb) *reinterpret_cast<float4*>(a.gout.dz_rgb + q * 4) = make_float4(v.dz[0], v.dz[1], v.dz[2], 0.0f);
}

// Pre-activation gradients of heads row `row` (0 density + normal head, 1 diff, 2 roughness, 3 tint) of point q; zero for INF.
template <bool FAST, class IDX>
__device__ __forceinline__ float4 head_grad_row(int row, const BwdJob& a, float density_bias, IDX q, float live, const HeadGradIn& v) {
  float4 qh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (a.mode == RSN_MODE_INF) return qh;
  if (row == 0) {
    const long long ray = (long long)(q / (IDX)a.S);
    const float rawd = a.fwd.raw_density[q];
    const float gs = a.gin.sigma ? a.gin.sigma[q] * live : 0.0f;
    qh.x = gs * FieldMath<FAST>::sigmoid(rawd + density_bias);  // softplus'
    // predicted normal: pn = normalize(-normalize(n_raw)); G = g_pn + g_ndd * dir
    float dir[3], G[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) dir[c] = a.directions[ray * 3 + c];
    if (a.gin.pred_normals) {
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c] = a.gin.pred_normals[q * 3 + c] * live;
    }
    float gd = a.gin.n_dot_d ? a.gin.n_dot_d[q] * live : 0.0f;
    if (a.gin.ray_pn_loss || a.gin.ray_ori_loss) {
      // fused normal losses (model.py:403-407): per-ray upstream gradients of sum_s w |n - n_pred|^2 and
      // sum_s w max(0, n.d)^2; the per-sample gradients are formed here and never stored
      const float w = a.gin.weights[q] * live;
      if (a.gin.ray_pn_loss) {
        const float gw = a.gin.ray_pn_loss[ray] * w * -2.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] += gw * (a.saved.normals[q * 3 + c] - a.fwd.pred_normals[q * 3 + c]);
      }
      if (a.gin.ray_ori_loss) gd += a.gin.ray_ori_loss[ray] * w * (2.0f * fmaxf(a.fwd.n_dot_d[q], 0.0f));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) G[c] += gd * dir[c];
    const float nraw[3] = {v.hd.x, v.hd.y, v.hd.z};
    const float len = fmaxf(sqrtf(nraw[0] * nraw[0] + nraw[1] * nraw[1] + nraw[2] * nraw[2]), 1e-12f);
    const float u[3] = {-(nraw[0] / len), -(nraw[1] / len), -(nraw[2] / len)};
    float gv[3], gu[3], gn[3];
    normalize_bwd(u, G, gv);
    gu[0] = -gv[0]; gu[1] = -gv[1]; gu[2] = -gv[2];
    normalize_bwd(nraw, gu, gn);
    qh.y = gn[0]; qh.z = gn[1]; qh.w = gn[2];
  } else if (row == 1) {
    qh.x = v.gcol[0] * (v.dif[0] * (1.0f - v.dif[0]));
    qh.y = v.gcol[1] * (v.dif[1] * (1.0f - v.dif[1]));
    qh.z = v.gcol[2] * (v.dif[2] * (1.0f - v.dif[2]));
  } else if (row == 2) {
    const float sr = FieldMath<FAST>::sigmoid(v.hd.w);
    const float gr = a.gin.roughness ? a.gin.roughness[q] * live : 0.0f;
    qh.x = gr * sr * (1.0f - sr);
  } else {
    qh.x = v.gcol[0] * v.mid[0] * (v.tin[0] * (1.0f - v.tin[0]));
    qh.y = v.gcol[1] * v.mid[1] * (v.tin[1] * (1.0f - v.tin[1]));
    qh.z = v.gcol[2] * v.mid[2] * (v.tin[2] * (1.0f - v.tin[2]));
  }
  return qh;
}

// Gradient w.r.t. the contracted Gaussian's variance -> the job's input (frustum: pixel_area; INF: sqradius), valid point q.
template <class IDX>
__device__ __forceinline__ float input_grad_of_dvar(const BwdJob& a, IDX q, const float (&dvar)[3]) {
  float g = 0.0f;
  if (a.mode == RSN_MODE_FRUSTUM) {
    const long long ray = (long long)(q / (IDX)a.S);
    const int s = (int)(q - (IDX)ray * (IDX)a.S);
    float o[3], d[3], dv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = a.origins[ray * 3 + c]; d[c] = a.directions[ray * 3 + c]; }
    frustum_dvar_dpa(o, d, a.pixel_area[ray], a.bins[ray * (a.S + 1) + s], a.bins[ray * (a.S + 1) + s + 1], dv);
    g = dvar[0] * dv[0] + dvar[1] * dv[1] + dvar[2] * dv[2];
  } else {  // INF: var_c = (0.6 sq)(1 - d_c^2)   (reflect_sampling_nerf_field.py:196)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float dc = a.directions[q * 3 + c];
      g += dvar[c] * (0.6f * (1.0f - dc * dc));
    }
  }
  return g;
}


// rsn_field_bf16_train.hip: the plain-bf16 training kernels on the LDS weight ring (width 256; rsn_ring_training())
int rsn_launch_field_bf16_train(long long n_tiles256, hipStream_t st, const FieldJobs& J);
int rsn_launch_field_bf16_bwd(long long n_tiles256, hipStream_t st, const BwdJobs& J);
// rsn_field_x6_train.hip: the split-bf16 (fp32-equivalent) training kernels on the LDS weight ring (width 256; 128-point tiles)
int rsn_launch_field_x6_train(long long n_tiles128, hipStream_t st, const FieldJobs& J);
int rsn_launch_field_x6_bwd(long long n_tiles128, hipStream_t st, const BwdJobs& J);
