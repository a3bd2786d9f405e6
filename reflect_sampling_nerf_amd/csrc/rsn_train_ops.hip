// rsn_train_ops.hip -- the two steps directly after the hot path in a training iteration:
//   rsn_loss_forward_backward : get_loss_dict (reflect_sampling_nerf_model.py:346-430) -- the 8 loss terms AND their
//                               gradients w.r.t. the model outputs in one pass over the samples;
//   rsn_radam_step            : RAdam (reference config.py:50-53 -> torch.optim.RAdam semantics) over all parameter
//                               tensors in one launch.
// Both are HBM-bound streaming kernels.
#include "rsn_common.h"

// ---------------------------------------------------------------------------------------------------
// losses.  Terms (index): 0 loss_mid_coarse, 1 loss_mid_fine, 2 loss_reflect_mid_coarse, 3 loss_reflect_mid_fine
// (MSE means over R*3), 4/5 predicted_normal_loss_{coarse,fine} = sum w |n - n_pred|^2, 6/7 orientation_loss_
// {coarse,fine} = sum w max(0, n.d)^2.  losses[k] receives the UNSCALED term; gradients are scaled by coef[k].
// ---------------------------------------------------------------------------------------------------
struct LossArgs {
  int R, Sc, Sf;
  const float* image;                       // [R,3] (already blended with the white background if RGBA)
  const float* rgb[4];                      // mid_rgb_coarse, mid_rgb_fine, mid_reflect_coarse, mid_reflect_fine [R,3]
  const float* w[2];                        // weights_coarse [R,Sc], weights_fine [R,Sf]   (detached)
  const float* nrm[2];                      // normals_* [R,S,3]                            (detached)
  const float* pn[2];                       // pred_normals_* [R,S,3]
  const float* ndd[2];                      // n_dot_d_* [R,S]
  float coef[8];
  float* losses;                            // [8], written by rsn_loss_reduce_kernel
  float* g_rgb[4];                          // [R,3]
  float* g_pn[2];                           // [R,S,3]
  float* g_ndd[2];                          // [R,S]
};

__device__ __forceinline__ double block_sum_256d(double v, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Per-block partial sums of the eight terms, owned by the library (one copy per device): the C ABI of rsn_loss_forward_backward
// has no workspace argument.  Written by every block of rsn_loss_kernel, read by rsn_loss_reduce_kernel in the same stream; two
// calls of rsn_loss_forward_backward on different streams of one device must not overlap.
#define LOSS_MAX_BLOCKS 1024
__device__ double rsn_loss_partials[LOSS_MAX_BLOCKS * 8];

__global__ __launch_bounds__(256) void rsn_loss_kernel(const LossArgs a) {
  __shared__ double shd[4];
  float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // MSE terms over R*3 elements
  const long long n3 = (long long)a.R * 3;
  const float inv = 1.0f / (float)n3;
  for (long long e = tid; e < n3; e += stride) {
    const float img = a.image[e];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dlt = a.rgb[k][e] - img;
      part[k] += dlt * dlt;
      if (a.g_rgb[k]) a.g_rgb[k][e] = a.coef[k] * 2.0f * dlt * inv;
    }
  }
  // per-sample terms
#pragma unroll
  for (int lv = 0; lv < 2; ++lv) {
    const long long n = (long long)a.R * (lv == 0 ? a.Sc : a.Sf);
    for (long long e = tid; e < n; e += stride) {
      const float w = a.w[lv][e];
      float s2 = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float dlt = a.nrm[lv][e * 3 + c] - a.pn[lv][e * 3 + c];
        s2 += dlt * dlt;
        if (a.g_pn[lv]) a.g_pn[lv][e * 3 + c] = a.coef[4 + lv] * w * (-2.0f * dlt);
      }
      part[4 + lv] += w * s2;
      const float nd = fmaxf(a.ndd[lv][e], 0.0f);
      part[6 + lv] += w * (nd * nd);
      if (a.g_ndd[lv]) a.g_ndd[lv][e] = a.coef[6 + lv] * w * (2.0f * nd);
    }
  }
  // this block's eight partial sums, in fp64 at a fixed position: rsn_loss_reduce_kernel adds the blocks' rows in a fixed order
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double v = block_sum_256d((double)part[k], shd);
    if (threadIdx.x == 0) rsn_loss_partials[blockIdx.x * 8 + k] = v;
  }
}

// One workgroup after rsn_loss_kernel (the launch boundary is the hand-off): losses[k] = sum over the blocks' rows, each thread
// over rows t, t + 256, ... in ascending order, then the fixed tree of block_sum_256d; one rounding to fp32.  Bit-reproducible.
__global__ __launch_bounds__(256) void rsn_loss_reduce_kernel(int blocks, double inv, float* losses) {
  __shared__ double shd[4];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) s += rsn_loss_partials[b * 8 + k];
    const double v = block_sum_256d(s, shd);
    if (threadIdx.x == 0) losses[k] = (float)(k < 4 ? v * inv : v);
  }
}

extern "C" int rsn_loss_forward_backward(int32_t n_rays, int32_t s_coarse, int32_t s_fine, const float* image,
                                         const float* const* rgb4, const float* const* weights2,
                                         const float* const* normals2, const float* const* pred_normals2,
                                         const float* const* n_dot_d2, const float* coef8, float* losses8,
                                         float* const* g_rgb4, float* const* g_pred_normals2, float* const* g_n_dot_d2,
                                         void* stream) {
  RSN_REQUIRE(n_rays >= 1 && s_coarse >= 1 && s_fine >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d s=%d,%d", n_rays,
              s_coarse, s_fine);
  RSN_REQUIRE(image && rgb4 && weights2 && normals2 && pred_normals2 && n_dot_d2 && coef8 && losses8 && g_rgb4 &&
                  g_pred_normals2 && g_n_dot_d2,
              RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  LossArgs a;
  a.R = n_rays; a.Sc = s_coarse; a.Sf = s_fine; a.image = image; a.losses = losses8;
  for (int k = 0; k < 4; ++k) { a.rgb[k] = rgb4[k]; a.g_rgb[k] = g_rgb4[k]; RSN_REQUIRE(rgb4[k], RSN_ERR_INVALID_ARGUMENT, "rgb[%d] NULL", k); }
  for (int k = 0; k < 2; ++k) {
    a.w[k] = weights2[k]; a.nrm[k] = normals2[k]; a.pn[k] = pred_normals2[k]; a.ndd[k] = n_dot_d2[k];
    a.g_pn[k] = g_pred_normals2[k]; a.g_ndd[k] = g_n_dot_d2[k];
    RSN_REQUIRE(a.w[k] && a.nrm[k] && a.pn[k] && a.ndd[k], RSN_ERR_INVALID_ARGUMENT, "level %d input NULL", k);
  }
  for (int k = 0; k < 8; ++k) a.coef[k] = coef8[k];
  hipStream_t st = (hipStream_t)stream;
  const long long work = (long long)n_rays * (s_coarse > s_fine ? s_coarse : s_fine);
  long long blocks = (work + 255) / 256;
  if (blocks > LOSS_MAX_BLOCKS) blocks = LOSS_MAX_BLOCKS;
  hipLaunchKernelGGL(rsn_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  RSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(rsn_loss_reduce_kernel, dim3(1), dim3(256), 0, st, (int)blocks, 1.0 / (double)((long long)n_rays * 3), losses8);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// In-place chain rule for the loss gradients: g_rgb[k] *= up[k] (k = 0..3), g_pn[lv] *= up[4 + lv], g_ndd[lv] *=
// up[6 + lv] with the eight upstream gradients d total / d loss_k read from DEVICE memory -- one launch instead of a
// dozen elementwise multiplications in the host framework's autograd.
struct LossScaleArgs {
  int R, Sc, Sf;
  const float* up;
  float* g_rgb[4];
  float* g_pn[2];
  float* g_ndd[2];
};

__global__ __launch_bounds__(256) void rsn_loss_scale_kernel(const LossScaleArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float up[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) up[k] = a.up[k];
  const long long n3 = (long long)a.R * 3;
  for (long long e = tid; e < n3; e += stride) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (a.g_rgb[k]) a.g_rgb[k][e] *= up[k];
  }
#pragma unroll
  for (int lv = 0; lv < 2; ++lv) {
    const long long n = (long long)a.R * (lv == 0 ? a.Sc : a.Sf);
    for (long long e = tid; e < n; e += stride) {
      if (a.g_pn[lv]) {
        a.g_pn[lv][e * 3 + 0] *= up[4 + lv];
        a.g_pn[lv][e * 3 + 1] *= up[4 + lv];
        a.g_pn[lv][e * 3 + 2] *= up[4 + lv];
      }
      if (a.g_ndd[lv]) a.g_ndd[lv][e] *= up[6 + lv];
    }
  }
}

extern "C" int rsn_loss_scale_grads(int32_t n_rays, int32_t s_coarse, int32_t s_fine, const float* upstream8,
                                    float* const* g_rgb4, float* const* g_pred_normals2, float* const* g_n_dot_d2,
                                    void* stream) {
  RSN_REQUIRE(n_rays >= 1 && s_coarse >= 1 && s_fine >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d s=%d,%d", n_rays,
              s_coarse, s_fine);
  RSN_REQUIRE(upstream8 && g_rgb4 && g_pred_normals2 && g_n_dot_d2, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  LossScaleArgs a;
  a.R = n_rays; a.Sc = s_coarse; a.Sf = s_fine; a.up = upstream8;
  for (int k = 0; k < 4; ++k) a.g_rgb[k] = g_rgb4[k];
  for (int k = 0; k < 2; ++k) { a.g_pn[k] = g_pred_normals2[k]; a.g_ndd[k] = g_n_dot_d2[k]; }
  const long long work = (long long)n_rays * (s_coarse > s_fine ? s_coarse : s_fine);
  long long blocks = (work + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(rsn_loss_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// ---------------------------------------------------------------------------------------------------
// get_loss_dict on per-ray quantities (training step): the per-sample normal terms arrive reduced per ray from the
// compositing epilogue (rsn_composite_io.pn_loss_ray / ori_loss_ray), so one small launch over R rays yields the eight
// terms and the gradients of the four colour terms; the chain rule is a second launch over R rays.
// ---------------------------------------------------------------------------------------------------
struct LossRaysArgs {
  int R;
  const float* image;
  const float* rgb[4];
  const float* pn_ray[2];
  const float* ori_ray[2];
  float coef[8];
  float* losses;
  float* g_rgb[4];
};

// ONE workgroup of 1024 threads: the eight reported loss values are reduced in a FIXED order (per-thread strided sums, a wave
// butterfly, the sixteen wave sums in index order) and are bit-reproducible from run to run -- the data is a few hundred KB,
// a second workgroup would only add float atomics whose arrival order varies (the gradients never depended on it).
__device__ __forceinline__ float block_sum_1024(float v, float* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  float t = 0.0f;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += sh[w];
  return t;
}

__global__ __launch_bounds__(1024) void rsn_loss_rays_kernel(const LossRaysArgs a) {
  __shared__ float sh[16];
  float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int stride = gridDim.x * blockDim.x;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int n3 = a.R * 3;
  const float inv = 1.0f / (float)n3;
  for (int e = tid; e < n3; e += stride) {
    const float img = a.image[e];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dlt = a.rgb[k][e] - img;
      part[k] += dlt * dlt;
      if (a.g_rgb[k]) a.g_rgb[k][e] = a.coef[k] * 2.0f * dlt * inv;
    }
  }
  for (int r = tid; r < a.R; r += stride) {
#pragma unroll
    for (int lv = 0; lv < 2; ++lv) {
      part[4 + lv] += a.pn_ray[lv][r];
      part[6 + lv] += a.ori_ray[lv][r];
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float v = block_sum_1024(part[k], sh);
    if (k < 4) v *= inv;
    if (threadIdx.x == 0) a.losses[k] = v;
  }
}

extern "C" int rsn_loss_rays_forward(int32_t n_rays, const float* image, const float* const* rgb4,
                                     const float* const* pn_loss_ray2, const float* const* ori_loss_ray2,
                                     const float* coef8, float* losses8, float* const* g_rgb4, void* stream) {
  RSN_REQUIRE(n_rays >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  RSN_REQUIRE(image && rgb4 && pn_loss_ray2 && ori_loss_ray2 && coef8 && losses8 && g_rgb4, RSN_ERR_INVALID_ARGUMENT,
              "a pointer is NULL");
  LossRaysArgs a;
  a.R = n_rays; a.image = image; a.losses = losses8;
  for (int k = 0; k < 4; ++k) { a.rgb[k] = rgb4[k]; a.g_rgb[k] = g_rgb4[k]; RSN_REQUIRE(rgb4[k], RSN_ERR_INVALID_ARGUMENT, "rgb[%d] NULL", k); }
  for (int k = 0; k < 2; ++k) {
    a.pn_ray[k] = pn_loss_ray2[k]; a.ori_ray[k] = ori_loss_ray2[k];
    RSN_REQUIRE(a.pn_ray[k] && a.ori_ray[k], RSN_ERR_INVALID_ARGUMENT, "level %d per-ray loss NULL", k);
  }
  for (int k = 0; k < 8; ++k) a.coef[k] = coef8[k];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rsn_loss_rays_kernel, dim3(1), dim3(1024), 0, st, a);  // one workgroup: fixed-order sums (see the kernel)
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

struct LossRaysBwdArgs {
  int R;
  const float* up;
  float coef[8];
  float* g_rgb[4];
  float* g_pn_ray[2];
  float* g_ori_ray[2];
};

__global__ __launch_bounds__(256) void rsn_loss_rays_bwd_kernel(const LossRaysBwdArgs a) {
  const int stride = gridDim.x * blockDim.x;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  float up[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) up[k] = a.up[k];
  for (int e = tid; e < a.R * 3; e += stride) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (a.g_rgb[k]) a.g_rgb[k][e] *= up[k];
  }
  for (int r = tid; r < a.R; r += stride) {
#pragma unroll
    for (int lv = 0; lv < 2; ++lv) {
      if (a.g_pn_ray[lv]) a.g_pn_ray[lv][r] = a.coef[4 + lv] * up[4 + lv];
      if (a.g_ori_ray[lv]) a.g_ori_ray[lv][r] = a.coef[6 + lv] * up[6 + lv];
    }
  }
}

extern "C" int rsn_loss_rays_backward(int32_t n_rays, const float* upstream8, const float* coef8, float* const* g_rgb4,
                                      float* const* g_pn_ray2, float* const* g_ori_ray2, void* stream) {
  RSN_REQUIRE(n_rays >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  RSN_REQUIRE(upstream8 && coef8 && g_rgb4 && g_pn_ray2 && g_ori_ray2, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  LossRaysBwdArgs a;
  a.R = n_rays; a.up = upstream8;
  for (int k = 0; k < 8; ++k) a.coef[k] = coef8[k];
  for (int k = 0; k < 4; ++k) a.g_rgb[k] = g_rgb4[k];
  for (int k = 0; k < 2; ++k) { a.g_pn_ray[k] = g_pn_ray2[k]; a.g_ori_ray[k] = g_ori_ray2[k]; }
  int blocks = (n_rays * 3 + 255) / 256;
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(rsn_loss_rays_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// ---------------------------------------------------------------------------------------------------
// RAdam, multi-tensor (torch.optim.RAdam: betas, eps, no weight decay, decoupled = false)
// ---------------------------------------------------------------------------------------------------
#define RADAM_MAX_TENSORS 48
struct RAdamArgs {
  float* p[RADAM_MAX_TENSORS];
  const float* g[RADAM_MAX_TENSORS];
  float* m[RADAM_MAX_TENSORS];
  float* v[RADAM_MAX_TENSORS];
  int n[RADAM_MAX_TENSORS];
  int n_tensors;
  float lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt, rect;  // rect < 0: variance not tractable yet (rho_t <= 5)
};

__global__ __launch_bounds__(256) void rsn_radam_kernel(const RAdamArgs a) {
  const int t = blockIdx.y;
  if (t >= a.n_tensors || a.g[t] == nullptr) return;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n[t]; i += gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float mi = a.beta1 * m[i] + (1.0f - a.beta1) * gi;   // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = a.beta2 * v[i] + (1.0f - a.beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / a.bias_c1;
    if (a.rect >= 0.0f) {
      const float adaptive = a.bias_c2_sqrt / (sqrtf(vi) + a.eps);
      p[i] = p[i] + mhat * a.lr * adaptive * a.rect * -1.0f;
    } else {
      p[i] = p[i] + mhat * a.lr * -1.0f;
    }
  }
}

extern "C" int rsn_radam_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int32_t* sizes, int32_t step, float lr, float beta1,
                              float beta2, float eps, void* stream) {
  RSN_REQUIRE(n_tensors >= 1 && n_tensors <= RADAM_MAX_TENSORS, RSN_ERR_INVALID_ARGUMENT, "n_tensors=%d (max %d)",
              n_tensors, RADAM_MAX_TENSORS);
  RSN_REQUIRE(params && grads && exp_avg && exp_avg_sq && sizes && step >= 1, RSN_ERR_INVALID_ARGUMENT,
              "a pointer is NULL or step < 1");
  RAdamArgs a;
  int max_n = 0;
  for (int t = 0; t < n_tensors; ++t) {
    a.p[t] = params[t]; a.g[t] = grads[t]; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t]; a.n[t] = sizes[t];
    RSN_REQUIRE(a.p[t] && a.m[t] && a.v[t] && a.n[t] >= 0, RSN_ERR_INVALID_ARGUMENT, "tensor %d has NULL state", t);
    if (a.n[t] > max_n) max_n = a.n[t];
  }
  a.n_tensors = n_tensors;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  // torch.optim.radam._single_tensor_radam, evaluated in double like Python does
  const double b1t = pow((double)beta1, (double)step), b2t = pow((double)beta2, (double)step);
  const double bias1 = 1.0 - b1t, bias2 = 1.0 - b2t;
  const double rho_inf = 2.0 / (1.0 - (double)beta2) - 1.0;
  const double rho_t = rho_inf - 2.0 * step * b2t / bias2;
  a.bias_c1 = (float)bias1;
  a.bias_c2_sqrt = (float)sqrt(bias2);
  a.rect = rho_t > 5.0
               ? (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
               : -1.0f;
  int bx = (max_n + 255) / 256;
  if (bx > 256) bx = 256;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(rsn_radam_kernel, dim3(bx, n_tensors), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// ---------------------------------------------------------------------------------------------------
// Guarded RAdam step (opt-in): global gradient-norm clipping and the skip of a step whose gradients hold an inf or a NaN.
// Two launches.  rsn_grad_sumsq_kernel leaves fp64 partial sums of squares at fixed positions, one per (tensor, block);
// rsn_radam_guarded_kernel sums them in a fixed order in every block's prologue (a few KB from L2: the launch boundary is the
// only hand-off between workgroups), derives the clip coefficient or the skip from the total, and applies rsn_radam_kernel's
// update to g * coef.  No atomics, no flag, no host read; the order of every sum is a function of (sizes, grid) alone.
// ---------------------------------------------------------------------------------------------------
#define GUARD_THREADS 256   // threads per block of both kernels
#define GUARD_VEC 4         // fp32 elements per vector load (16 bytes)
#define GUARD_SLOTS 8       // most blocks (= partial sums) per tensor: 48 x 8 doubles = 3 KB read per prologue

struct GradSumsqArgs {
  const float* g[RADAM_MAX_TENSORS];
  int n[RADAM_MAX_TENSORS];
  double* partials;  // [n_tensors][GUARD_SLOTS]; block (s, t) writes slot t * GUARD_SLOTS + s
};

// Block (s, t) of a (slots, n_tensors) grid.  Tensor t is cut into quads of GUARD_VEC consecutive elements; thread k of the
// slots * GUARD_THREADS threads of the row takes quads k, k + slots * GUARD_THREADS, ... and adds their squares element by
// element, in fp64 (the square of an fp32 value is exact there); threads 0 .. n % GUARD_VEC - 1 then take one element of the
// tail each.  A 16-byte aligned tensor reads its quads as float4, any other one element by element: the same sums either way.
__global__ __launch_bounds__(GUARD_THREADS) void rsn_grad_sumsq_kernel(const GradSumsqArgs a) {
  __shared__ double sh[GUARD_THREADS / 64];
  const int t = blockIdx.y;
  const float* __restrict__ g = a.g[t];
  if (g == nullptr) return;  // no slot of this tensor is read
  const int n = a.n[t];
  const int nq = n / GUARD_VEC;
  const int k = blockIdx.x * GUARD_THREADS + threadIdx.x;
  const int stride = gridDim.x * GUARD_THREADS;
  double acc = 0.0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (int q = k; q < nq; q += stride) {
      const float4 x = g4[q];
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    }
  } else {
    for (int q = k; q < nq; q += stride) {
#pragma unroll
      for (int e = 0; e < GUARD_VEC; ++e) {
        const double x = (double)g[(size_t)q * GUARD_VEC + e];
        acc += x * x;
      }
    }
  }
  if (k < n - nq * GUARD_VEC) {
    const double x = (double)g[(size_t)nq * GUARD_VEC + k];
    acc += x * x;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partials[t * GUARD_SLOTS + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// blocks along x that rsn_grad_sumsq launches (and rsn_radam_step_guarded reads) for these sizes
static int guard_slots(int32_t n_tensors, const int32_t* sizes) {
  int max_n = 0;
  for (int t = 0; t < n_tensors; ++t)
    if (sizes[t] > max_n) max_n = sizes[t];
  const int per_block = GUARD_THREADS * GUARD_VEC;
  int slots = max_n / per_block + (max_n % per_block != 0);
  if (slots > GUARD_SLOTS) slots = GUARD_SLOTS;
  return slots < 1 ? 1 : slots;
}

extern "C" size_t rsn_grad_sumsq_workspace_bytes(int32_t n_tensors, const int32_t* sizes) {
  if (n_tensors < 1 || n_tensors > RADAM_MAX_TENSORS || !sizes) {
    rsn_set_error("n_tensors=%d (max %d) or sizes NULL", n_tensors, RADAM_MAX_TENSORS);
    return 0;
  }
  return (size_t)n_tensors * GUARD_SLOTS * sizeof(double);
}

extern "C" int rsn_grad_sumsq(int32_t n_tensors, const float* const* grads, const int32_t* sizes, void* workspace,
                              size_t workspace_bytes, void* stream) {
  RSN_REQUIRE(n_tensors >= 1 && n_tensors <= RADAM_MAX_TENSORS, RSN_ERR_INVALID_ARGUMENT, "n_tensors=%d (max %d)",
              n_tensors, RADAM_MAX_TENSORS);
  RSN_REQUIRE(grads && sizes && workspace, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  RSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, RSN_ERR_INVALID_ARGUMENT, "workspace is not 8-byte aligned");
  const size_t need = (size_t)n_tensors * GUARD_SLOTS * sizeof(double);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "workspace of %zu bytes, needs %zu", workspace_bytes, need);
  GradSumsqArgs a;
  for (int t = 0; t < n_tensors; ++t) {
    RSN_REQUIRE(sizes[t] >= 0, RSN_ERR_INVALID_ARGUMENT, "tensor %d has size %d", t, sizes[t]);
    a.g[t] = grads[t]; a.n[t] = sizes[t];
  }
  a.partials = (double*)workspace;
  hipLaunchKernelGGL(rsn_grad_sumsq_kernel, dim3(guard_slots(n_tensors, sizes), n_tensors), dim3(GUARD_THREADS), 0,
                     (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

struct RAdamGuardArgs {
  RAdamArgs r;
  const double* partials;  // what rsn_grad_sumsq left: [n_tensors][GUARD_SLOTS], `slots` of each row written
  int slots;
  int step;
  float max_norm;          // <= 0: no clipping
  int skip_nonfinite;
  rsn_guard_stats* stats;
};

__global__ __launch_bounds__(256) void rsn_radam_guarded_kernel(const RAdamGuardArgs a) {
  __shared__ double sh_sq[RADAM_MAX_TENSORS];
  __shared__ double sh_total;
  const int t = blockIdx.y;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;  // the block that records the statistics, update or not
  const bool idle = a.r.g[t] == nullptr || (int)(blockIdx.x * blockDim.x) >= a.r.n[t];
  if (idle && !first) return;
  // every block forms the same total from the same partial sums in the same order: per tensor over its slots, then over the
  // tensors in index order
  if (threadIdx.x < RADAM_MAX_TENSORS) {
    double s = 0.0;
    if ((int)threadIdx.x < a.r.n_tensors && a.r.g[threadIdx.x] != nullptr)
      for (int k = 0; k < a.slots; ++k) s += a.partials[threadIdx.x * GUARD_SLOTS + k];
    sh_sq[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < a.r.n_tensors; ++k) s += sh_sq[k];
    sh_total = s;
  }
  __syncthreads();
  const double total_sq = sh_total;
  const float norm = (float)sqrt(total_sq);
  const bool skip = a.skip_nonfinite != 0 && !isfinite(total_sq);
  float coef = 1.0f;
  if (a.max_norm > 0.0f) {  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1), a NaN stays a NaN
    const float c = a.max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  if (first) {
    rsn_guard_stats* st = a.stats;
    if (threadIdx.x < RADAM_MAX_TENSORS) {
      st->per_tensor_sq[threadIdx.x] = sh_sq[threadIdx.x];
      if (skip) st->per_tensor_sq_at_last_skip[threadIdx.x] = sh_sq[threadIdx.x];
    }
    if (threadIdx.x == 0) {
      st->last_norm = norm;
      st->last_coef = coef;
      st->last_skipped = skip ? 1 : 0;
      if (skip) {
        st->skipped_total = st->skipped_total + 1;
        st->last_skipped_step = a.step;
      }
    }
  }
  if (skip || idle) return;
  float* __restrict__ p = a.r.p[t];
  const float* __restrict__ g = a.r.g[t];
  float* __restrict__ m = a.r.m[t];
  float* __restrict__ v = a.r.v[t];
  // rsn_radam_kernel's loop on g[i] * coef (coef = 1: the same bits, x * 1.0f is exact)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.r.n[t]; i += gridDim.x * blockDim.x) {
    const float gi = g[i] * coef;
    const float mi = a.r.beta1 * m[i] + (1.0f - a.r.beta1) * gi;
    const float vi = a.r.beta2 * v[i] + (1.0f - a.r.beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / a.r.bias_c1;
    if (a.r.rect >= 0.0f) {
      const float adaptive = a.r.bias_c2_sqrt / (sqrtf(vi) + a.r.eps);
      p[i] = p[i] + mhat * a.r.lr * adaptive * a.r.rect * -1.0f;
    } else {
      p[i] = p[i] + mhat * a.r.lr * -1.0f;
    }
  }
}

extern "C" int rsn_radam_step_guarded(int32_t n_tensors, float* const* params, const float* const* grads,
                                      float* const* exp_avg, float* const* exp_avg_sq, const int32_t* sizes, int32_t step,
                                      float lr, float beta1, float beta2, float eps, float max_norm, int32_t skip_nonfinite,
                                      const void* workspace, size_t workspace_bytes, rsn_guard_stats* stats, void* stream) {
  RSN_REQUIRE(n_tensors >= 1 && n_tensors <= RADAM_MAX_TENSORS, RSN_ERR_INVALID_ARGUMENT, "n_tensors=%d (max %d)",
              n_tensors, RADAM_MAX_TENSORS);
  RSN_REQUIRE(params && grads && exp_avg && exp_avg_sq && sizes && step >= 1, RSN_ERR_INVALID_ARGUMENT,
              "a pointer is NULL or step < 1");
  RSN_REQUIRE(workspace && stats, RSN_ERR_INVALID_ARGUMENT, "workspace or stats is NULL");
  RSN_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(stats)) & 7) == 0,
              RSN_ERR_INVALID_ARGUMENT, "workspace or stats is not 8-byte aligned");
  RSN_REQUIRE(max_norm == max_norm, RSN_ERR_INVALID_ARGUMENT, "max_norm is NaN");
  const size_t need = (size_t)n_tensors * GUARD_SLOTS * sizeof(double);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "workspace of %zu bytes, needs %zu", workspace_bytes, need);
  RAdamGuardArgs a;
  int max_n = 0;
  for (int t = 0; t < n_tensors; ++t) {
    a.r.p[t] = params[t]; a.r.g[t] = grads[t]; a.r.m[t] = exp_avg[t]; a.r.v[t] = exp_avg_sq[t]; a.r.n[t] = sizes[t];
    RSN_REQUIRE(a.r.p[t] && a.r.m[t] && a.r.v[t] && a.r.n[t] >= 0, RSN_ERR_INVALID_ARGUMENT, "tensor %d has NULL state", t);
    if (a.r.n[t] > max_n) max_n = a.r.n[t];
  }
  a.r.n_tensors = n_tensors;
  a.r.lr = lr; a.r.beta1 = beta1; a.r.beta2 = beta2; a.r.eps = eps;
  // the step-dependent factors exactly as rsn_radam_step forms them
  const double b1t = pow((double)beta1, (double)step), b2t = pow((double)beta2, (double)step);
  const double bias1 = 1.0 - b1t, bias2 = 1.0 - b2t;
  const double rho_inf = 2.0 / (1.0 - (double)beta2) - 1.0;
  const double rho_t = rho_inf - 2.0 * step * b2t / bias2;
  a.r.bias_c1 = (float)bias1;
  a.r.bias_c2_sqrt = (float)sqrt(bias2);
  a.r.rect = rho_t > 5.0
                 ? (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
                 : -1.0f;
  a.partials = (const double*)workspace;
  a.slots = guard_slots(n_tensors, sizes);
  a.step = step;
  a.max_norm = (max_norm > 0.0f && max_norm <= 3.402823466e+38f) ? max_norm : 0.0f;  // <= 0 or +inf: no clipping
  a.skip_nonfinite = skip_nonfinite != 0;
  a.stats = stats;
  int bx = (max_n + 255) / 256;
  if (bx > 256) bx = 256;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(rsn_radam_guarded_kernel, dim3(bx, n_tensors), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// ------------------------------------------------------------------------------------------------
// rsn_unfold_bottleneck_grads: the folded training step (RSN_MMA_F32_FOLDED) reduces C = sum d a_mid (x) act[L-1] and s = sum d a_mid
// over the points; the parameter gradients of field_output_bottleneck and of the x part of mlp_mid.layers.0 follow from them exactly:
//   dW_b = W_mx^T C      db_b = W_mx^T s      dW_mx = C W_b^T + s (x) b_b          (W_mx = mid_w[:, 34:])
// One thread per output element, fp64 products summed in ascending index order, one fp32 rounding, one fp32 add: bit-reproducible.
// ------------------------------------------------------------------------------------------------
struct UnfoldArgs {
  int w, n_mid, ld_c, ld_mid;
  const float* c; const float* s; const float* mid_w; const float* bott_w; const float* bott_b;
  float* d_bott_w; float* d_bott_b; float* d_mid_w;
};

__global__ __launch_bounds__(256) void rsn_unfold_kernel(const UnfoldArgs a) {
  const int w = a.w, n_mid = a.n_mid;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  const float* __restrict__ wmx = a.mid_w + RSN_SH_DIM;
  if (e < w * w) {  // dW_b[k][j] += sum_i W_mx[i][k] C[i][j]
    const int k = e / w, j = e - k * w;
    double acc = 0.0;
    for (int i = 0; i < n_mid; ++i) acc += (double)wmx[(size_t)i * a.ld_mid + k] * (double)a.c[(size_t)i * a.ld_c + j];
    a.d_bott_w[e] += (float)acc;
    return;
  }
  e -= w * w;
  if (e < w) {  // db_b[k] += sum_i W_mx[i][k] s[i]
    double acc = 0.0;
    for (int i = 0; i < n_mid; ++i) acc += (double)wmx[(size_t)i * a.ld_mid + e] * (double)a.s[i];
    a.d_bott_b[e] += (float)acc;
    return;
  }
  e -= w;
  if (e < n_mid * w) {  // dW_mx[i][k] += sum_j C[i][j] W_b[k][j] + s[i] b_b[k]
    const int i = e / w, k = e - i * w;
    double acc = 0.0;
    for (int j = 0; j < w; ++j) acc += (double)a.c[(size_t)i * a.ld_c + j] * (double)a.bott_w[(size_t)k * w + j];
    acc += (double)a.s[i] * (double)a.bott_b[k];
    a.d_mid_w[(size_t)i * a.ld_mid + RSN_SH_DIM + k] += (float)acc;
  }
}

extern "C" int rsn_unfold_bottleneck_grads(int32_t width, int32_t n_mid, const float* c, int32_t ld_c, const float* s,
                                           const float* mid_w, int32_t ld_mid, const float* bott_w, const float* bott_b,
                                           float* d_bott_w, float* d_bott_b, float* d_mid_w, void* stream) {
  RSN_REQUIRE(width >= 1 && width <= 256 && n_mid >= 1 && n_mid <= 1024, RSN_ERR_INVALID_ARGUMENT, "width=%d (1..256) n_mid=%d (1..1024)",
              width, n_mid);
  RSN_REQUIRE(ld_c >= width && ld_mid >= RSN_SH_DIM + width, RSN_ERR_INVALID_ARGUMENT, "ld_c=%d < width=%d or ld_mid=%d < %d + width",
              ld_c, width, ld_mid, RSN_SH_DIM);
  RSN_REQUIRE(c && s && mid_w && bott_w && bott_b && d_bott_w && d_bott_b && d_mid_w, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  UnfoldArgs a = {width, n_mid, ld_c, ld_mid, c, s, mid_w, bott_w, bott_b, d_bott_w, d_bott_b, d_mid_w};
  const int n = width * width + width + n_mid * width;
  hipLaunchKernelGGL(rsn_unfold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
