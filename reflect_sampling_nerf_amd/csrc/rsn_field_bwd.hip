// rsn_field_bwd.hip -- backward sweep of the field for one sampling level (training).
//
// Mirror image of rsn_field.hip: one wavefront owns 32 sample points and walks the network backwards with the
// TRANSPOSED packed weights (rsn_pack.hip, wT_* segments).  dX[k][m] = sum_n W[n][k] * dY[n][m] has the same
// "A = weights, B = points" shape as the forward GEMM, so the lane-local trick carries over unchanged: the
// accumulator registers a lane holds after one W^T GEMM are (after the ReLU mask) the B operand it needs for the
// next one.  ReLU masks come from the post-ReLU activations the training forward saved (x > 0).
//
// What leaves the kernel are the PRE-ACTIVATION gradients of every linear layer, row-major [N, out_features]:
// the weight gradients dW = dY^T X (contraction over all N samples) and the bias gradients are taken by
// rsn_weight_grad (rsn_wgrad.hip).
//
// Autograd semantics restated (reference: reflect_sampling_nerf_model.py:142-344, field.py:122-207):
//   colour = diff + tint * mid          -> d diff = g, d tint = g*mid, d mid = g*tint
//   SH inputs carry no gradient (components.py:52, roughness.detach() at model.py:174)
//   pred_normals = normalize(-normalize(head))      n_dot_d = sum(dir * pred_normals)
//   sigma = softplus(raw + density_bias)            roughness (rendered) = sum w * sigmoid(raw)
//   reflect levels: the Gaussian covariance depends on pixel_area = pi * sqradius (a function of the NON-detached
//   rendered roughness, model.py:225-227,272,286), so the gradient w.r.t. the encoded inputs' variance is carried
//   back to pixel_area (need_input_grad).
#include "rsn_epilogues.h"
#include "rsn_field_bwd_common.h"

// FOLD (RSN_MMA_F32_FOLDED, see rsn_field_kernel.h): stages 2 and 3 are ONE GEMM d emb = [W_c ; W_heads]^T [d a_mid ; dz_heads] over
// K = 128 + 32; no bottleneck gradient row exists (gout.d_bott is neither written nor read).
// MMA: the rsn_mma_mode the kernel serves (MmaTraits, rsn_gemm_loops.h); MODE = the mode whose K loops it runs.
template <int NB, int MMA>
__global__ __launch_bounds__(256) void rsn_field_bwd_kernel(const BwdJobs J) {
  using M = MmaTraits<MMA>;
  constexpr bool FOLD = M::FOLD;
  constexpr int MODE = M::LOOPS;
  constexpr int HIT = FOLD ? 16 : NB * 4;  // first K-iteration of the heads gradients in the slab (FOLD: behind d a_mid's 16)
  constexpr int XITS = (NB * 4 > 16) ? NB * 4 : 16;
  constexpr int WAVE_F4 = (XITS + RSN_AUX_ITS) * 64;
  constexpr int W = NB * 32;
  constexpr bool SBF = M::SAVE_BF16;  // reduced-precision training: wide layer gradients (dy, d_bott, da_mid) stored as bf16
  __shared__ float4 smem[4 * WAVE_F4];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // a SCALAR (tile bases, buffer descriptors)
  float4* X = smem + wid * WAVE_F4 + lane;  // its XITS.. spill into the SH region (contiguous): NB*4+4 <= XITS+5
  float* Xf = reinterpret_cast<float*>(X);

  const BwdShared& P = J.s;
  const TileJobs T = tile_space<128>(J);
  const float* __restrict__ pk = P.packed;
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

  for (long long gtile = blockIdx.x; gtile < T.n_tiles; gtile += gridDim.x) {
    const TileAt ta = tile_at(T, gtile);  // workgroup-uniform
    const BwdJob& a = J.j[ta.job];
    const long long n_points = ta.n_points, tile = ta.tile;
    const long long p0 = tile * 128 + wid * 32;
    if (p0 >= n_points) continue;
    // opaque per-tile copy of the lane id: keeps hipcc from hoisting (and spilling) per-lane addresses out of the loop
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int m = ln & 31, h = ln >> 5;
    const long long p = p0 + m;
    const bool valid = p < n_points;
    const long long pc = valid ? p : n_points - 1;
    const int rows = (int)(n_points - p0 < 32 ? n_points - p0 : 32);  // valid rows of this wave's tile (wave-uniform)
    // Layer-gradient rows kept for the weight gradients.  Exact fp32: a row leaves from the K loop of the GEMM that READS it
    // (one buffer store per K-iteration, gemm_run2's `save`); the split / plain bf16 loops store from the epilogue that
    // produces it.  History: with the two-buffer K loop this arrangement ran the sweeps 12.1 -> 12.5 ms per step (vmcnt
    // counts stores in order with the loads, so a fragment wait also waited out the store in front of it); with the
    // fragments two iterations ahead (gemm_run2) it is 11.78 -> 11.55 ms.
    constexpr bool LOOPST = M::LOOP_STORES;
    auto rb_epi = [&](float* base, long long elem, int row_elems) {
      return rowbuf<SBF>(LOOPST ? nullptr : base, elem, rows, row_elems, m, h);
    };
    auto rb_loop = [&](float* base, long long elem, int row_elems) {
      return rowbuf<false>(LOOPST ? base : nullptr, elem, rows, row_elems, m, h);
    };
    const float live = valid ? 1.0f : 0.0f;  // padded lanes contribute zero gradients

    auto bits_at = [&](int l) -> const unsigned* {  // rsn_field_saved.relu_bits: [L+1][N][2][NB/2] words
      return a.saved.relu_bits + ((((long long)l * (a.act_stride / W)) + pc) * 2 + h) * (NB / 2 > 2 ? NB / 2 : 2);
    };
    // ---------------- per-sample epilogue gradients -----------------
    HeadGradIn hg;
    head_grad_inputs(a, pc, live, h == 1 && valid, hg);

    // ---------------- stage 1: d hidden = W_rgb^T dz  (K = 32 with rows 4..6 live), ReLU mask -----------------
    X[0] = (h == 1) ? make_float4(hg.dz[0], hg.dz[1], hg.dz[2], 0.0f) : zero4;
    X[64] = zero4; X[128] = zero4; X[192] = zero4;
    {
      const ReluBits<4> mb = load_relu_bits<4>(bits_at(P.num_layers));
      __builtin_amdgcn_sched_barrier(0);
      f32x16 acc[4];
      zero_acc<4>(acc);
      gemm_mode<MODE, 4, 4, true>(acc, pk + P.L.wT_rgb, pk + P.L.hT_rgb, X, 4, ln);
      store_masked_bits<4, SBF>(acc, X, mb, h, rb_epi(a.gout.da_mid, p0 * 128, 128));
    }
    // ---------------- stage 2: d bottleneck = W_mid[:, 34:]^T d a_mid -----------------
    if constexpr (!FOLD) {
      f32x16 acc[NB];
      zero_acc<NB>(acc);
      gemm_mode<MODE, NB, NB, true>(acc, pk + P.L.wT_mid_x, pk + P.L.hT_mid_x, X, 16, ln, rb_loop(a.gout.da_mid, p0 * 128, 128));
      store_act<NB, NB, false, SBF>(acc, X, rb_epi(a.gout.d_bott, p0 * W, W), h);
    }
    // ---------------- stage 3: heads pre-activation gradients, then d emb = [W_b; W_heads]^T [d b; dz_heads] ------
    {
      // heads rows 8q + 4h + j for q = 0, 1: this half's two rows, h and h + 2
      const float4 q0 = head_grad_row<false>(h == 0 ? 0 : 1, a, P.density_bias, pc, live, hg);
      const float4 q1 = head_grad_row<false>(h == 0 ? 2 : 3, a, P.density_bias, pc, live, hg);
      X[(HIT + 0) * 64] = q0;
      X[(HIT + 1) * 64] = q1;
      X[(HIT + 2) * 64] = zero4;
      X[(HIT + 3) * 64] = zero4;
      if (valid && a.gout.dz_heads) {
        *reinterpret_cast<float4*>(a.gout.dz_heads + pc * 16 + 4 * h) = q0;
        *reinterpret_cast<float4*>(a.gout.dz_heads + pc * 16 + 8 + 4 * h) = q1;
      }
      const int l = P.num_layers - 1;
      const ReluBits<NB> mb = load_relu_bits<NB>(bits_at(l));
      __builtin_amdgcn_sched_barrier(0);
      f32x16 acc[NB];
      zero_acc<NB>(acc);
      if constexpr (FOLD)  // reads (and keeps) d a_mid: its rows end at K-iteration 16, the heads gradients behind them are not stored
        gemm_mode<MODE, NB, NB, true>(acc, pk + P.L.wT_fold, pk + P.L.hT_bh, X, 16 + 4, ln, rb_loop(a.gout.da_mid, p0 * 128, 128));
      else
        gemm_mode<MODE, NB, NB, true>(acc, pk + P.L.wT_bh, pk + P.L.hT_bh, X, NB * 4 + 4, ln, rb_loop(a.gout.d_bott, p0 * W, W));
      store_masked_bits<NB, SBF>(acc, X, mb, h, rb_epi(a.gout.dy, (long long)l * a.act_stride + p0 * W, W));
    }
    // ---------------- stage 4: trunk, layers L-1 .. 1 -----------------
    // FOLD: the W x W GEMMs run on the bf16 MFMAs as all nine products of three bf16 pieces a side, on the 16x16x32 shape, from the
    // packed pieces the analytic-normal sweep of the training forward reads (rsn_field_kernel.h; hT_last: those of layer L-1):
    // exact fp32 products, another order of the fp32 accumulation.  Stages 1 to 3 left the slab in its standard layout, which is
    // what that loop reads.  A lane reads and writes float4 of other lanes' slots there (in order within the wave: no barrier), so
    // the saved rows leave for the rows of the two points it reads (rb16) and the mask words are those of the two it writes.
    // (Nine here, where the analytic-normal sweep takes six: with six, d_input missed its rule -- DESIGN 4.3.)
    // The two encoded-input GEMMs stay on the fp32 loop (they read the same slab): on the nine-product loop d_input missed the rule
    // of tests/test_layer_gemms_gpu.py in two cases.
    f32x16 eacc[4];
    zero_acc<4>(eacc);
    auto rb16 = [&](float* base, long long elem, int row_elems) {
      return rowbuf<false>(base, elem, rows, row_elems, ln & 15, (ln >> 4) & 1);
    };
    auto bits16_at = [&](int l, int ph) -> const unsigned* {  // the old lane (ln & 15) + 16 ph + 32 ((ln >> 4) & 1)
      const long long q = p0 + (ln & 15) + 16 * ph, qc = q < n_points ? q : n_points - 1;
      return a.saved.relu_bits + ((((long long)l * (a.act_stride / W)) + qc) * 2 + ((ln >> 4) & 1)) * (NB / 2 > 2 ? NB / 2 : 2);
    };
#pragma unroll 1
    for (int l = P.num_layers - 1; l >= 1; --l) {
      if (a.need_input_grad && l == P.skip_layer)
        gemm_mode<MODE, 4, 4, true>(eacc, pk + P.L.wT_enc_skip, pk + P.L.hT_enc_skip, X, NB * 4, ln);
      if constexpr (FOLD) {
        const ReluBits<NB> mb[2] = {load_relu_bits<NB>(bits16_at(l - 1, 0)), load_relu_bits<NB>(bits16_at(l - 1, 1))};
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[NB][2][2];
        zero_acc16<NB>(acc);
        gemm_bf16_s16<NB, 9>(acc, pk + (l == P.num_layers - 1 ? (size_t)P.L.hT_last : P.L.hT_x[l]), X, NB, ln,
                             rb16(a.gout.dy, (long long)l * a.act_stride + p0 * W, W));  // reads (and keeps) dy[l]
        store_masked_bits16<NB>(acc, X, mb, ln);
      } else {
        const ReluBits<NB> mb = load_relu_bits<NB>(bits_at(l - 1));
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[NB];
        zero_acc<NB>(acc);
        gemm_mode<MODE, NB, NB, true>(acc, pk + P.L.wT_x[l], pk + P.L.hT_x[l], X, NB * 4, ln,
                            rb_loop(a.gout.dy, (long long)l * a.act_stride + p0 * W, W));  // reads (and keeps) dy[l]
        store_masked_bits<NB, SBF>(acc, X, mb, h, rb_epi(a.gout.dy, (long long)(l - 1) * a.act_stride + p0 * W, W));
      }
    }
    if (LOOPST && !a.need_input_grad) {  // dy[0] has no GEMM behind it on this path: its rows leave here
      const RowBuf r0 = rb_loop(a.gout.dy, p0 * W, W);
#pragma unroll 4
      for (int it = 0; it < NB * 4; ++it) sv_put_it(r0, it, X[it * 64]);
    }
    // ---------------- stage 5: gradient w.r.t. the Gaussian's variance -> pixel_area / sqradius -----------------
    if (a.need_input_grad) {
      gemm_mode<MODE, 4, 4, true>(eacc, pk + P.L.wT_enc0, pk + P.L.hT_enc0, X, NB * 4, ln, rb_loop(a.gout.dy, p0 * W, W));  // keeps dy[0]
      store_act<4, 4, false>(eacc, X);  // d loss / d encoded input, slot order
      const float* encp = a.saved.enc + pc * RSN_K_ENC_PAD;
      float dvar[3];
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        float part = 0.0f;
#pragma unroll 2
        for (int jj = 0; jj < 8; ++jj) {
          const float f = h ? P.freqs[8 + jj] : P.freqs[jj];
          const int u = c * 8 + jj, u2 = u + 24;
          const float gs = Xf[(u >> 2) * 256 + (u & 3)], gc = Xf[(u2 >> 2) * 256 + (u2 & 3)];
          const float fs = encp[(u >> 2) * 8 + 4 * h + (u & 3)], fc = encp[(u2 >> 2) * 8 + 4 * h + (u2 & 3)];
          part += (-0.5f * (f * f)) * (gs * fs + gc * fc);  // d/dvar [exp(-var f^2/2) sin(.)] = -f^2/2 * feature
        }
        const float tot = part + __shfl_xor(part, 32, 64);
        if (c == 0) dvar[0] = tot; else if (c == 1) dvar[1] = tot; else dvar[2] = tot;
      }
      if (h == 0 && valid && a.gout.d_input) a.gout.d_input[pc] = input_grad_of_dvar(a, pc, dvar);
    }
  }
}

// One launch over the backward sweeps of n evaluations of one field.
static int launch_bwd_jobs(const rsn_field_desc* d, const float* packed, BwdJob* js, int n, void* stream) {
  RSN_REQUIRE(n >= 1 && n <= RSN_MAX_JOBS, RSN_ERR_INVALID_ARGUMENT, "n_jobs=%d (1..%d)", n, RSN_MAX_JOBS);
  BwdJobs J = {};
  RSN_TRY(rsn_fill_shared(J.s, d, packed));
  for (int k = 0; k < n; ++k) {
    BwdJob& a = js[k];
    RSN_REQUIRE(a.saved.relu_bits && a.saved.heads && a.gout.dy, RSN_ERR_INVALID_ARGUMENT,
                "job %d: saved relu_bits / heads and gout.dy are required", k);
    RSN_REQUIRE(!a.need_input_grad || (a.saved.enc && a.gout.d_input), RSN_ERR_INVALID_ARGUMENT,
                "job %d: need_input_grad needs saved.enc and gout.d_input", k);
    RSN_REQUIRE(a.mode == RSN_MODE_INF || (a.fwd.raw_density && a.fwd.diff && a.fwd.tint), RSN_ERR_INVALID_ARGUMENT,
                "job %d: forward values raw_density/diff/tint are required", k);
    RSN_REQUIRE(!(a.gin.ray_pn_loss || a.gin.ray_ori_loss) || (a.mode == RSN_MODE_FRUSTUM && a.gin.weights),
                RSN_ERR_INVALID_ARGUMENT, "job %d: fused normal losses need the level's weights (frustum levels only)", k);
    RSN_REQUIRE(!a.gin.ray_pn_loss || (a.saved.normals && a.fwd.pred_normals), RSN_ERR_INVALID_ARGUMENT,
                "job %d: ray_pn_loss needs saved.normals and the forward pred_normals", k);
    RSN_REQUIRE(!a.gin.ray_ori_loss || a.fwd.n_dot_d, RSN_ERR_INVALID_ARGUMENT, "job %d: ray_ori_loss needs the forward n_dot_d", k);
    if (a.n_rays <= 0) continue;
    a.act_stride = (long long)a.n_rays * a.S * (long long)d->width;
    J.j[J.n_jobs++] = a;
  }
  if (J.n_jobs == 0) return RSN_OK;
  const long long n_tiles = rsn_job_tiles(J, 128);
  const int cached_cus = rsn_device_cus();
  const long long grid = n_tiles < (long long)cached_cus ? n_tiles : (long long)cached_cus;
  hipStream_t st = (hipStream_t)stream;
  const bool x6 = d->mma_mode == RSN_MMA_BF16X6;  // fp32-emulating split-bf16 sweeps (opt-in); else exact fp32
  if (rsn_ring_training(d))  // plain / split bf16 training at width 256: the LDS-ring kernels (256- / 128-point tiles)
    return x6 ? rsn_launch_field_x6_bwd(n_tiles, st, J) : rsn_launch_field_bf16_bwd(rsn_job_tiles(J, 256), st, J);
  RSN_TRY(rsn_for_width(d->width, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    const dim3 g((unsigned)grid), b(256);
    if (x6) hipLaunchKernelGGL((rsn_field_bwd_kernel<NB, RSN_MMA_BF16X6>), g, b, 0, st, J);
    else if (d->mma_mode == RSN_MMA_BF16)  // reduced-precision training sweeps (bf16 operands, fp32 accumulate)
      hipLaunchKernelGGL((rsn_field_bwd_kernel<NB, RSN_MMA_BF16>), g, b, 0, st, J);
    else if (d->mma_mode == RSN_MMA_F32_FOLDED)  // exact fp32, the bottleneck folded into mlp_mid
      hipLaunchKernelGGL((rsn_field_bwd_kernel<NB, RSN_MMA_F32_FOLDED>), g, b, 0, st, J);
    else hipLaunchKernelGGL((rsn_field_bwd_kernel<NB, RSN_MMA_F32>), g, b, 0, st, J);
  }));
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

static int launch_bwd(const rsn_field_desc* d, const float* pk, BwdJob& a, void* st) { return launch_bwd_jobs(d, pk, &a, 1, st); }

// The entry points: NULL-check the struct pointers, fill a zeroed BwdJob with the kind's filler (rsn_field_common.h, shared with
// the forward) and the gradient blocks, launch; what the sweeps require of those blocks is checked once, in launch_bwd_jobs.
extern "C" int rsn_field_backward_jobs(const rsn_field_desc* desc, const float* packed, int32_t n_jobs,
                                       const rsn_field_bwd_job* jobs, void* stream) {
  RSN_REQUIRE(desc && jobs, RSN_ERR_INVALID_ARGUMENT, "desc/jobs is NULL");
  RSN_REQUIRE(n_jobs >= 1 && n_jobs <= RSN_MAX_JOBS, RSN_ERR_INVALID_ARGUMENT, "n_jobs=%d (1..%d)", n_jobs, RSN_MAX_JOBS);
  BwdJob js[RSN_MAX_JOBS] = {};
  for (int k = 0; k < n_jobs; ++k) {
    const rsn_field_bwd_job& q = jobs[k];
    BwdJob& a = js[k];
    const JobPrefix pfx(k);
    RSN_REQUIRE(q.kind == 0 || q.kind == 1, RSN_ERR_INVALID_ARGUMENT, "job %d: kind=%d", k, q.kind);
    RSN_REQUIRE(q.n_rays >= 0 && q.saved && q.gout, RSN_ERR_INVALID_ARGUMENT, "job %d: n_rays / saved / gout", k);
    if (q.kind == 0) {
      RSN_REQUIRE(q.n_samples >= 1 && q.fwd && q.gin, RSN_ERR_INVALID_ARGUMENT, "job %d: n_samples / fwd / gin", k);
      RSN_TRY(rsn_fill_frustum(a, pfx.s, q.n_rays, q.n_dev, q.n_samples, q.origins, q.directions, q.pixel_area, q.euclid_bins));
      a.gin = *q.gin; a.fwd = *q.fwd;
    } else {
      RSN_TRY(rsn_fill_inf(a, pfx.s, q.n_rays, q.n_dev, q.directions, q.sqradius, q.g_rgb));
      a.gin.color = q.g_rgb;
    }
    a.need_input_grad = q.need_input_grad;
    a.saved = *q.saved; a.gout = *q.gout;
  }
  return launch_bwd_jobs(desc, packed, js, n_jobs, stream);
}

extern "C" int rsn_field_backward_frustum(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                          const int32_t* n_dev, int32_t n_samples, const float* origins,
                                          const float* directions, const float* pixel_area, const float* euclid_bins,
                                          const rsn_field_outputs* fwd, const rsn_field_saved* saved,
                                          const rsn_field_grads_in* gin, const rsn_field_grads_out* gout,
                                          int32_t need_input_grad, void* stream) {
  RSN_REQUIRE(desc && fwd && saved && gin && gout, RSN_ERR_INVALID_ARGUMENT, "a struct pointer is NULL");
  RSN_REQUIRE(n_rays >= 0 && n_samples >= 1, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d n_samples=%d", n_rays, n_samples);
  BwdJob a = {};
  RSN_TRY(rsn_fill_frustum(a, "", n_rays, n_dev, n_samples, origins, directions, pixel_area, euclid_bins));
  a.need_input_grad = need_input_grad;
  a.gin = *gin; a.fwd = *fwd; a.saved = *saved; a.gout = *gout;
  return launch_bwd(desc, packed, a, stream);
}

extern "C" int rsn_field_backward_inf(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                      const int32_t* n_dev, const float* directions, const float* sqradius,
                                      const rsn_field_saved* saved, const float* g_rgb,
                                      const rsn_field_grads_out* gout, int32_t need_input_grad, void* stream) {
  RSN_REQUIRE(desc && saved && gout, RSN_ERR_INVALID_ARGUMENT, "a struct pointer is NULL");
  RSN_REQUIRE(n_rays >= 0, RSN_ERR_INVALID_ARGUMENT, "n_rays=%d", n_rays);
  BwdJob a = {};
  RSN_TRY(rsn_fill_inf(a, "", n_rays, n_dev, directions, sqradius, g_rgb));
  a.need_input_grad = need_input_grad;
  a.gin.color = g_rgb;
  a.saved = *saved; a.gout = *gout;
  return launch_bwd(desc, packed, a, stream);
}
