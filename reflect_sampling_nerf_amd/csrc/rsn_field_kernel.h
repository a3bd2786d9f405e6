// rsn_field_kernel.h -- the field kernel template (see rsn_field.hip for the layout argument), shared by two translation
// units that differ in ONE compiler flag (reflect_sampling_nerf_amd/_build.py, SOURCE_FLAGS):
//   rsn_field.hip        exact fp32 (RSN_MMA_F32, RSN_MMA_F32_FOLDED) and plain-bf16 training (RSN_MMA_BF16): MFMA accumulators in
//                        architected VGPRs (-amdgpu-mfma-vgpr-form: the epilogues touch every accumulator; no v_accvgpr copies, no
//                        scratch -- but for the two NB = 8 exact-fp32 training kernels, which hold both trunk paths: DESIGN 4.3);
//   rsn_field_split.hip  split-bf16 (RSN_MMA_BF16X6, RSN_MMA_BF16X3): hipcc's default AGPR accumulators -- these kernels also hold
//                        the bf16 triples of the operands, and in VGPR form their training forward runs 14 % slower.
// The K loops are rsn_gemm_loops.h (with MmaTraits: what a mode means), the epilogues rsn_epilogues.h.
#pragma once
#include "rsn_epilogues.h"
#include "rsn_field_common.h"

// ------------------------------------------------------------------------------------------------
// FOLD (exact-fp32 training, RSN_MMA_F32_FOLDED): field_output_bottleneck has no activation and feeds only the x part of
// mlp_mid.layers.0, so the two are ONE affine map W_c = W_mx W_b, b_c = b_mid + W_mx b_b (rsn_fold_kernel, rsn_pack.hip).  The
// N = W + 32 GEMM over the trunk output becomes N = 128 + 32 (the four mlp_mid blocks, started from b_c, and the heads block), the
// SH part then accumulates into the same four blocks, and the K = W GEMM over the bottleneck row is gone with the row itself
// (saved.bott is neither written nor read).  Heads, sigma and normals keep their bits: same K order, same bias start.
// MMA: the rsn_mma_mode the kernel serves (MmaTraits, rsn_gemm_loops.h); MODE = the mode whose K loops it runs.
// A loop GEMM of the analytic-normal sweep in the mode's own loop, and, for the exact-fp32 training instantiations, as the
// piece-product loop on the 16x16x32 bf16 MFMAs: PACKED (FOLD) over the pre-split hT_* segment, else with the same pieces formed in
// registers from the fp32 wT_* segment (the RSN_MMA_F32 buffer has no split copies): the same bits either way.
template <int MODE, int NBO>
__device__ __forceinline__ void sweep_gemm(f32x16 (&acc)[NBO], const float* __restrict__ w32, const float* __restrict__ w16,
                                           const float4* xl, int n_it, int lane) {
  gemm_mode<MODE, NBO, NBO, true>(acc, w32, w16, xl, n_it, lane);
}
// The W x W GEMMs of the training forward's trunk (layers l >= 1, the x part) go the same way, over h_x[l] / w_x[l], with `save`:
// the rows of act[l-1] leave from the K loop that reads them.
// NP: the piece products per accumulator and K step (rsn_gemm_loops.h): 9 in the trunk, 6 in the analytic-normal sweep.
template <bool PACKED, int N_IT, int NBO, int NP, class SV = const float*>
__device__ __forceinline__ void sweep_gemm(f32x4 (&acc)[NBO][2][2], const float* __restrict__ w32, const float* __restrict__ w16,
                                           const float4* xl, int lane, SV save = nullptr) {
  static_assert(N_IT % 4 == 0, "K = 8 N_IT is a multiple of 32 at every width (the units are padded to 32): no tail path");
  if constexpr (PACKED) gemm_bf16_s16<NBO, NP>(acc, w16, xl, N_IT / 4, lane, save);
  else gemm_f32_s16<NBO, NP>(acc, w32, xl, N_IT / 4, lane, save);
}

template <int NB, bool TRAIN, int MMA>
__global__ __launch_bounds__(256) void rsn_field_kernel(const FieldJobs J) {
  using M = MmaTraits<MMA>;
  constexpr bool FOLD = M::FOLD;
  constexpr int MODE = M::LOOPS;
  static_assert(!FOLD || TRAIN, "the folded bottleneck serves the exact-fp32 training kernels");
  constexpr int NBH = FOLD ? 5 : NB + 1;  // row blocks of the GEMM that carries the heads block (its last)
  constexpr int XITS = (NB * 4 > 16) ? NB * 4 : 16;  // >= 14 (encoding, K=16 steps) and >= 16 (mid hidden)
  constexpr int WAVE_F4 = (XITS + RSN_AUX_ITS) * 64;
  constexpr int W = NB * 32;
  constexpr bool SBF = TRAIN && M::SAVE_BF16;  // reduced-precision training: activations / bottleneck / mid hidden saved as bf16
  __shared__ float4 smem[4 * WAVE_F4];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // a SCALAR: tile bases / buffer descriptors derive from it
  float4* X = smem + wid * WAVE_F4 + lane;
  float4* AUX = X + XITS * 64;
  float* Xf = reinterpret_cast<float*>(X);

  const FieldShared& P = J.s;
  const TileJobs T = tile_space<128>(J);
  const float* __restrict__ pk = P.packed;

  for (long long gtile = blockIdx.x; gtile < T.n_tiles; gtile += gridDim.x) {
    const TileAt ta = tile_at(T, gtile);  // workgroup-uniform
    const FieldJob& a = J.j[ta.job];
    const long long n_points = ta.n_points, tile = ta.tile;
    const long long p0 = tile * 128 + wid * 32;
    if (p0 >= n_points) continue;  // wave-uniform; waves never synchronise with each other
    // an opaque copy of the lane id per tile: per-lane weight / output addresses are then not loop-invariant, so hipcc
    // cannot hoist dozens of them out of the persistent tile loop and spill them to scratch
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int m = ln & 31, h = ln >> 5;
    const long long p = p0 + m;
    const bool valid = p < n_points;
    const long long pc = valid ? p : n_points - 1;
    const int rows = (int)(n_points - p0 < 32 ? n_points - p0 : 32);  // valid rows of this wave's tile (wave-uniform)
    // Saved rows (training).  Exact fp32: a row leaves from the K loop of the GEMM that READS it (one store per
    // K-iteration, gemm_run); the split / plain bf16 loops store from the epilogue that produces it.
    constexpr bool LOOPST = TRAIN && M::LOOP_STORES;
    auto rb_epi = [&](float* base, long long elem, int row_elems) {
      return rowbuf<SBF>((TRAIN && !LOOPST) ? base : nullptr, elem, rows, row_elems, m, h);
    };
    auto rb_loop = [&](float* base, long long elem, int row_elems) {
      return rowbuf<false>(LOOPST ? base : nullptr, elem, rows, row_elems, m, h);
    };
    // training: this lane's slot in the ReLU bit masks of layer l (rsn_field_saved.relu_bits: [L+1][N][2][NB/2] words)
    auto bits_at = [&](int l) -> unsigned* {
      return a.saved.relu_bits + ((((long long)l * (a.act_stride / W)) + pc) * 2 + h) * (NB / 2 > 2 ? NB / 2 : 2);
    };

    float mc[3] = {0.0f, 0.0f, 0.0f}, vc[3] = {0.0f, 0.0f, 0.0f}, vd[3] = {0.0f, 0.0f, 0.0f};
    bool has_cov = true, has_dir = true;
    float4 wbh[NBH];  // first weight fragment of the bottleneck+heads GEMM
    const float* __restrict__ w_bh = pk + (FOLD ? P.L.w_fold : P.L.w_bh);
    if (a.mode == RSN_MODE_EMB) {
      pre_mode<MODE, NBH>(wbh, w_bh, ln);
      // granular Field API: heads / mid MLP on a caller-supplied embedding (field.py:139-186)
      has_dir = a.view_dirs != nullptr;
#pragma unroll
      for (int c = 0; c < 3; ++c) vd[c] = has_dir ? a.view_dirs[pc * 3 + c] : 0.0f;
#pragma unroll 4
      for (int it = 0; it < NB * 4; ++it)
        X[it * 64] = *reinterpret_cast<const float4*>(a.emb_in + pc * W + it * 8 + 4 * h);
    } else {
    // ---------------- encode -----------------
    if (a.mode == RSN_MODE_FRUSTUM || a.mode == RSN_MODE_INF) {
      has_dir = point_gaussian(a, pc, mc, vc, vd);
    } else {
      has_cov = a.cov_diag != nullptr;
      has_dir = a.view_dirs != nullptr;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mc[c] = a.means[pc * 3 + c];
        vc[c] = has_cov ? a.cov_diag[pc * 3 + c] : 0.0f;
        vd[c] = has_dir ? a.view_dirs[pc * 3 + c] : 0.0f;
      }
    }

    // integrated positional encoding (nerfstudio NeRFEncoding, N2): this lane produces the features of
    // frequencies 8h..8h+7 into its own LDS slots (slot order: rsn_pack.hip enc_slot_to_column).
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      const float x = (c == 0) ? mc[0] : (c == 1 ? mc[1] : mc[2]);
      const float v = (c == 0) ? vc[0] : (c == 1 ? vc[1] : vc[2]);
      const float sx = 6.283185307179586f * x;
#pragma unroll 2
      for (int jj = 0; jj < 8; ++jj) {
        const float f = h ? P.freqs[8 + jj] : P.freqs[jj];
        const float ang = sx * f;
        const float e = has_cov ? expf(-0.5f * (v * (f * f))) : 1.0f;
        const float fs = e * sin_big(ang);
        const float fc = e * sin_big(ang + 1.5707963267948966f);
        const int u = c * 8 + jj;
        Xf[(u >> 2) * 256 + (u & 3)] = fs;
        Xf[((u + 24) >> 2) * 256 + ((u + 24) & 3)] = fc;
      }
    }
    {
      float4 raw = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (h == 0) raw = make_float4(mc[0], mc[1], mc[2], 0.0f);
      X[12 * 64] = raw;
      if (!M::F32) X[13 * 64] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // K=16 steps read iteration 13 (zero weights)
    }
    // this lane's 52 encoded inputs, re-used by the skip layer.  Held as vector-typed SSA values (not an
    // indexable array) so that they stay in the unified VGPR/AGPR file instead of scratch memory.
    f32x16 st0, st1, st2;
    float4 st3;
    {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const float4 t0 = X[it * 64], t1 = X[(4 + it) * 64], t2 = X[(8 + it) * 64];
        st0[4 * it + 0] = t0.x; st0[4 * it + 1] = t0.y; st0[4 * it + 2] = t0.z; st0[4 * it + 3] = t0.w;
        st1[4 * it + 0] = t1.x; st1[4 * it + 1] = t1.y; st1[4 * it + 2] = t1.z; st1[4 * it + 3] = t1.w;
        st2[4 * it + 0] = t2.x; st2[4 * it + 1] = t2.y; st2[4 * it + 2] = t2.z; st2[4 * it + 3] = t2.w;
      }
      st3 = X[12 * 64];
    }
    if (TRAIN && a.saved.enc && valid) {  // [N,104] in slot order
      float* row = a.saved.enc + pc * RSN_K_ENC_PAD;
#pragma unroll
      for (int it = 0; it < RSN_ENC_ITS; ++it) *reinterpret_cast<float4*>(row + it * 8 + 4 * h) = X[it * 64];
    }

    // ---------------- trunk -----------------
    // Exact-fp32 training (RSN_MMA_F32 and RSN_MMA_F32_FOLDED): the W x W GEMM of every layer l >= 1 (its x part) runs as nine bf16
    // products on the 16x16x32 shape (sweep_gemm: FOLD over the packed pieces h_x[l], else the same pieces formed in registers from
    // w_x[l] -- the same bits), its accumulators started from the bias in that shape's layout (init_acc16) and left through
    // store_act16_relu, which writes the slab and the mask words exactly where store_act does.  Layer 0 and the encoded-input part
    // of the skip layer stay on the fp32 loop (K = 104 is no multiple of 32).  The skip layer's x part moves too: its accumulators
    // change layout once through the wave's own slab (store_act16, load_acc) before the encoded-input GEMM adds to them.
    // The jobs of a training step take this path (conical frustums, get_inf_color).  The explicit-Gaussian job of the granular
    // Field API keeps the fp32 loop (workgroup-uniform branch): get_density(.., requires_density_grad) hands out the bits of the
    // plain forward, which runs the eval kernel (tests/test_gpu_parity.py holds the two equal).
    bool s16 = false;
    if constexpr (TRAIN && M::F32) s16 = a.mode == RSN_MODE_FRUSTUM || a.mode == RSN_MODE_INF;
    if (s16) {
     if constexpr (TRAIN && M::F32) {
      // the mask words this lane stores from the 16-shape: point (L & 15) + 16 (L >> 5), half (L >> 4) & 1 (store_act16_relu)
      auto bits16_st = [&](int l) -> unsigned* {
        const long long q = p0 + (ln & 15) + 16 * (ln >> 5);
        if (!a.saved.relu_bits || q >= n_points) return nullptr;
        return a.saved.relu_bits + ((((long long)l * (a.act_stride / W)) + q) * 2 + ((ln >> 4) & 1)) * (NB / 2 > 2 ? NB / 2 : 2);
      };
      auto rb_loop16 = [&](float* base, long long elem, int row_elems) {
        return rowbuf<false>(base, elem, rows, row_elems, ln & 15, (ln >> 4) & 1);
      };
      {
        f32x16 acc[NB];
        float4 wpre[NB];
        pre_mode<MODE, NB>(wpre, pk + P.L.w_enc0, ln);
        init_acc<NB>(acc, pk + P.L.b[0], h);
        gemm_mode_run<MODE, NB, NB, TRAIN>(acc, wpre, pk + P.L.w_enc0, pk + P.L.h_enc0, X, RSN_ENC_ITS, ln);
        if (P.num_layers == 1) pre_mode<MODE, NBH>(wbh, w_bh, ln);
        store_act<NB, NB, true, false>(acc, X, rb_epi(a.saved.act, p0 * W, W), h, (a.saved.relu_bits && valid) ? bits_at(0) : nullptr);
      }
      if (P.num_layers > 1) {
        f32x4 a16[NB][2][2];
        init_acc16<NB>(a16, pk + P.L.b[1], ln);
#pragma unroll 1
        for (int l = 1; l < P.num_layers; ++l) {
          sweep_gemm<FOLD, NB * 4, NB, 9>(a16, pk + P.L.w_x[l], pk + P.L.h_x[l], X, ln,
                                       rb_loop16(a.saved.act, (l - 1) * a.act_stride + p0 * W, W));
          const bool last = l + 1 == P.num_layers;
          if (l == P.skip_layer) {
            f32x16 acc[NB];
            float4 wpre[NB];
            pre_mode<MODE, NB>(wpre, pk + P.L.w_enc_skip, ln);
            store_act16<NB>(a16, X, ln);
            load_acc<NB>(acc, X);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              X[it * 64] = make_float4(st0[4 * it], st0[4 * it + 1], st0[4 * it + 2], st0[4 * it + 3]);
              X[(4 + it) * 64] = make_float4(st1[4 * it], st1[4 * it + 1], st1[4 * it + 2], st1[4 * it + 3]);
              X[(8 + it) * 64] = make_float4(st2[4 * it], st2[4 * it + 1], st2[4 * it + 2], st2[4 * it + 3]);
            }
            X[12 * 64] = st3;
            gemm_mode_run<MODE, NB, NB, TRAIN>(acc, wpre, pk + P.L.w_enc_skip, pk + P.L.h_enc_skip, X, RSN_ENC_ITS, ln);
            if (last) pre_mode<MODE, NBH>(wbh, w_bh, ln);
            store_act<NB, NB, true, false>(acc, X, rb_epi(a.saved.act, p0 * W, W), h,
                                           (a.saved.relu_bits && valid) ? bits_at(l) : nullptr);
            if (!last) init_acc16<NB>(a16, pk + P.L.b[l + 1], ln);
          } else if (!last) {
            store_act16_relu_init<NB>(a16, X, ln, pk + P.L.b[l + 1], bits16_st(l));
          } else {
            pre_mode<MODE, NBH>(wbh, w_bh, ln);
            store_act16_relu<NB>(a16, X, ln, bits16_st(l));
          }
        }
      }
     }
    } else {
      f32x16 acc[NB];
      float4 wpre[NB];  // first weight fragment of the next GEMM, fetched ahead of the epilogue in front of it
      pre_mode<MODE, NB>(wpre, pk + P.L.w_enc0, ln);
      init_acc<NB>(acc, pk + P.L.b[0], h);
      gemm_mode_run<MODE, NB, NB, TRAIN>(acc, wpre, pk + P.L.w_enc0, pk + P.L.h_enc0, X, RSN_ENC_ITS, ln);
#pragma unroll 1
      for (int l = 1; l < P.num_layers; ++l) {
        pre_mode<MODE, NB>(wpre, pk + P.L.w_x[l], ln);
        // ReLU between layers; the accumulators restart from layer l's bias
        store_act_init<NB, true, SBF>(acc, X, rb_epi(a.saved.act, (l - 1) * a.act_stride + p0 * W, W),
                                 h, pk + P.L.b[l], (TRAIN && a.saved.relu_bits && valid) ? bits_at(l - 1) : nullptr);
        gemm_mode_run<MODE, NB, NB, TRAIN>(acc, wpre, pk + P.L.w_x[l], pk + P.L.h_x[l], X, NB * 4, ln,
                                rb_loop(a.saved.act, (l - 1) * a.act_stride + p0 * W, W));
        if (l == P.skip_layer) {
          pre_mode<MODE, NB>(wpre, pk + P.L.w_enc_skip, ln);
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            X[it * 64] = make_float4(st0[4 * it], st0[4 * it + 1], st0[4 * it + 2], st0[4 * it + 3]);
            X[(4 + it) * 64] = make_float4(st1[4 * it], st1[4 * it + 1], st1[4 * it + 2], st1[4 * it + 3]);
            X[(8 + it) * 64] = make_float4(st2[4 * it], st2[4 * it + 1], st2[4 * it + 2], st2[4 * it + 3]);
          }
          X[12 * 64] = st3;
          if (!M::F32) X[13 * 64] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          gemm_mode_run<MODE, NB, NB, TRAIN>(acc, wpre, pk + P.L.w_enc_skip, pk + P.L.h_enc_skip, X, RSN_ENC_ITS, ln);
        }
      }
      // out_activation = ReLU
      pre_mode<MODE, NBH>(wbh, w_bh, ln);
      store_act<NB, NB, true, SBF>(acc, X, rb_epi(a.saved.act, (P.num_layers - 1) * a.act_stride + p0 * W, W), h,
                              (TRAIN && a.saved.relu_bits && valid) ? bits_at(P.num_layers - 1) : nullptr);
    }
    }  // mode != RSN_MODE_EMB
    if (a.embedding && valid) {
#pragma unroll 4
      for (int it = 0; it < NB * 4; ++it)
        *reinterpret_cast<float4*>(a.embedding + pc * W + it * 8 + 4 * h) = X[it * 64];
    }

    // ---------------- bottleneck + heads (one GEMM, N = W + 32) -----------------
    float dcol[3], tcol[3], rho;
    float4 wmid[4];  // first weight fragment of mlp_mid's SH part
    f32x16 accm[4];  // mlp_mid's pre-activation (FOLD: its x part comes out of the GEMM below, started from b_c)
    {
      f32x16 acc[NBH];
      init_acc<NBH>(acc, pk + (FOLD ? P.L.b_fold : P.L.b_bh), h);
      gemm_mode_run<MODE, NBH, NBH, TRAIN>(acc, wbh, w_bh, pk + P.L.h_bh, X, NB * 4, ln,
                                  rb_loop(a.mode == RSN_MODE_EMB ? nullptr : a.saved.act, (P.num_layers - 1) * a.act_stride + p0 * W, W));
      pre_mode<MODE, 4>(wmid, pk + P.L.w_mid_sh, ln);
      const float r0 = acc[NBH - 1][0], r1 = acc[NBH - 1][1], r2 = acc[NBH - 1][2], r3 = acc[NBH - 1][3];
      const float r4 = acc[NBH - 1][4], r5 = acc[NBH - 1][5], r6 = acc[NBH - 1][6];
      // h == 0: r0 raw density, r1..r3 normals, r4 roughness.   h == 1: r0..r2 diff, r4..r6 tint.
      const float rough_raw = __shfl(r4, m, 64);
      rho = (a.mode == RSN_MODE_EMB && a.rough_in) ? a.rough_in[pc] : softplus_f(rough_raw);
      dcol[0] = sigmoid_f(r0); dcol[1] = sigmoid_f(r1); dcol[2] = sigmoid_f(r2);
      tcol[0] = sigmoid_f(r4); tcol[1] = sigmoid_f(r5); tcol[2] = sigmoid_f(r6);
      if (valid) {  // rows h and h + 2 of the heads
        head_outputs_row<false, false>(h == 0 ? 0 : 1, a, P.density_bias, pc, make_float4(r0, r1, r2, r3), dcol, vd);
        head_outputs_row<false, false>(h == 0 ? 2 : 3, a, P.density_bias, pc, make_float4(r4, r5, r6, 0.0f), tcol, vd);
        // raw normal head (3) + raw roughness head: both rows sit in this lane, so their saved.heads share leaves as ONE store
        if (TRAIN && a.saved.heads && h == 0) *reinterpret_cast<float4*>(a.saved.heads + pc * 8) = make_float4(r1, r2, r3, r4);
      }
      if constexpr (FOLD) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) accm[nb] = acc[nb];
      } else {
        // bottleneck output (no activation) becomes the x-part of mlp_mid's input
        store_act<NBH, NB, false, SBF>(acc, X, rb_epi(a.saved.bott, p0 * W, W), h);
      }
    }

    // ---------------- SH-34 of the view direction, attenuated by softplus roughness -----------------
    {
      float sh[34];
      if (has_dir) {
        sh34_attenuated(vd[0], vd[1], vd[2], rho, sh);
      } else {
#pragma unroll
        for (int i = 0; i < 34; ++i) sh[i] = 0.0f;
      }
#pragma unroll
      for (int it = 0; it < RSN_SH_ITS; ++it) {
        float vals[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int u = it * 4 + s;
          vals[s] = (u < 17) ? (h ? sh[17 + u] : sh[u]) : 0.0f;
        }
        AUX[it * 64] = make_float4(vals[0], vals[1], vals[2], vals[3]);
        if (!M::F32 && it == 0) AUX[5 * 64] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (TRAIN && a.saved.sh && valid)
          *reinterpret_cast<float4*>(a.saved.sh + pc * RSN_K_SH_PAD + it * 8 + 4 * h) =
              make_float4(vals[0], vals[1], vals[2], vals[3]);
      }
    }

    // ---------------- mlp_mid + RGB head -----------------
    float4 wrgb[1];
    {
      if constexpr (FOLD) {  // the SH part on top of W_c a + b_c
        gemm_mode_run<MODE, 4, 4, TRAIN>(accm, wmid, pk + P.L.w_mid_sh, pk + P.L.h_mid_sh, AUX, RSN_SH_ITS, ln);
      } else {
        init_acc<4>(accm, pk + P.L.b_mid, h);
        float4 wmx[4];
        pre_mode<MODE, 4>(wmx, pk + P.L.w_mid_x, ln);
        gemm_mode_run<MODE, 4, 4, TRAIN>(accm, wmid, pk + P.L.w_mid_sh, pk + P.L.h_mid_sh, AUX, RSN_SH_ITS, ln);
        gemm_mode_run<MODE, 4, 4, TRAIN>(accm, wmx, pk + P.L.w_mid_x, pk + P.L.h_mid_x, X, NB * 4, ln, rb_loop(a.saved.bott, p0 * W, W));
      }
      pre_mode<MODE, 1>(wrgb, pk + P.L.w_rgb, ln);
      store_act<4, 4, true, SBF>(accm, X, rb_epi(a.saved.hid, p0 * 128, 128), h,
                            (TRAIN && a.saved.relu_bits && valid) ? bits_at(P.num_layers) : nullptr);
    }
    {
      f32x16 accr[1];
      init_acc<1>(accr, pk + P.L.b_rgb, h);
      gemm_mode_run<MODE, 1, 1, TRAIN>(accr, wrgb, pk + P.L.w_rgb, pk + P.L.h_rgb, X, 16, ln, rb_loop(a.saved.hid, p0 * 128, 128));
      if (h == 1 && valid) colour_out<false, TRAIN>(a, pc, accr[0][0], accr[0][1], accr[0][2], dcol, tcol);
    }

    // ---------------- training: analytic normals = -normalize(d raw_density / d contracted mean) -----------------
    // (reflect_sampling_nerf_field.py:125-127,146-147 -> nerfstudio Field.get_normals).  A dX-only sweep back
    // through the trunk: seed = density-head row masked by the embedding's ReLU, then W_l^T GEMMs masked by the
    // saved activations; the encoded-input gradient accumulates in 4 extra blocks (slot order), and the chain
    // through sin(2 pi x f [+ pi/2]) * exp(-var f^2 / 2) is closed per lane (the covariance is a constant here,
    // exactly like the reference, which sets requires_grad on the mean after contraction).
    // Exact fp32 (RSN_MMA_F32 and RSN_MMA_F32_FOLDED): the first GEMM of the sweep, W_{L-1}^T (w_density masked by the bits of
    // layer L-1), runs on the bf16 MFMAs straight from those bits against V = W_{L-1}^T diag(w_density) in three bf16 pieces: the
    // peeled iteration l = L-1.  FOLD reads the pieces packed (hT_seed, gemm_bf16_bits); RSN_MMA_F32, whose packed buffer has no
    // such segment, forms them in registers (gemm_f32_bits): the same bits.  The skip layer is never the last one
    // (rsn_compute_layout), so that iteration has no encoded-input GEMM.
    // The GEMMs behind it (W_l^T for l = L-2 .. 1 and the two encoded-input GEMMs) run on the bf16 MFMAs too, as SIX products of
    // three bf16 pieces a side (sweep_gemm, SWEEP_NP): the three smallest of the nine, at most 2^-25 of the product each, are left
    // out -- below the rounding of the fp32 accumulation they would join, and no sign is decided from these sums (rsn_gemm_loops.h).
    // They run on the 16x16x32 shape (rsn_gemm_loops.h): a lane then reads and writes float4 of OTHER lanes' slots of the wave's X
    // slab, which needs no barrier -- a wave's LDS instructions complete in order, and no other wave touches the slab.
    constexpr bool SEED_BITS = TRAIN && M::F32;
    [[maybe_unused]] constexpr int SWEEP_NP = 6;  // piece products per accumulator and K step of the sweep's loop GEMMs, folded and unfolded alike
    if (TRAIN && a.saved.normals && a.saved.relu_bits) {
      const float* __restrict__ wd = pk + P.L.v_density;
      const bool peel = SEED_BITS && P.num_layers >= 2;  // workgroup-uniform
      if (peel) {
        const ReluBits<NB> m7 = load_relu_bits<NB>(bits_at(P.num_layers - 1));
        const ReluBits<NB> mb = load_relu_bits<NB>(bits_at(P.num_layers - 2));
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[NB];
        zero_acc<NB>(acc);
        if constexpr (FOLD) {
          gemm_bf16_bits<NB>(acc, pk + P.L.hT_seed, m7, ln);
        } else {  // RSN_MMA_F32: no packed seed, the same pieces formed in registers (same bits)
          gemm_f32_bits<NB>(acc, pk + P.L.wT_x[P.num_layers - 1], wd, m7, ln);
        }
        store_masked_bits<NB>(acc, X, mb, h);
      } else {
        // seed: the density-head row masked by the embedding's ReLU (bits of the last trunk layer)
        const ReluBits<NB> mb = load_relu_bits<NB>(bits_at(P.num_layers - 1));
#pragma unroll
        for (int it = 0; it < NB * 4; ++it) {
          const float4 w = *reinterpret_cast<const float4*>(wd + it * 8 + 4 * h);
          const int word = mb.w[it / 8];
          const int base = ((it / 4) & 1) * 16 + 4 * (it & 3);
          X[it * 64] = make_float4(
              __uint_as_float(__float_as_uint(w.x) & bit_mask(word, base + 0)),
              __uint_as_float(__float_as_uint(w.y) & bit_mask(word, base + 1)),
              __uint_as_float(__float_as_uint(w.z) & bit_mask(word, base + 2)),
              __uint_as_float(__float_as_uint(w.w) & bit_mask(word, base + 3)));
        }
      }
      if constexpr (SEED_BITS) {
        // the mask words of the two old lanes whose float4 this lane writes (store_masked_bits16): point halves 0 and 1
        auto bits16_at = [&](int l, int ph) -> const unsigned* {
          const long long q = p0 + (ln & 15) + 16 * ph, qc = q < n_points ? q : n_points - 1;
          return a.saved.relu_bits + ((((long long)l * (a.act_stride / W)) + qc) * 2 + ((ln >> 4) & 1)) * (NB / 2 > 2 ? NB / 2 : 2);
        };
        f32x4 eacc[4][2][2];
        zero_acc16<4>(eacc);
#pragma unroll 1
        for (int l = P.num_layers - (peel ? 2 : 1); l >= 1; --l) {
          if (l == P.skip_layer) sweep_gemm<FOLD, NB * 4, 4, SWEEP_NP>(eacc, pk + P.L.wT_enc_skip, pk + P.L.hT_enc_skip, X, ln);
          const ReluBits<NB> mb[2] = {load_relu_bits<NB>(bits16_at(l - 1, 0)), load_relu_bits<NB>(bits16_at(l - 1, 1))};
          __builtin_amdgcn_sched_barrier(0);
          f32x4 acc[NB][2][2];
          zero_acc16<NB>(acc);
          sweep_gemm<FOLD, NB * 4, NB, SWEEP_NP>(acc, pk + P.L.wT_x[l], pk + P.L.hT_x[l], X, ln);
          store_masked_bits16<NB>(acc, X, mb, ln);
        }
        sweep_gemm<FOLD, NB * 4, 4, SWEEP_NP>(eacc, pk + P.L.wT_enc0, pk + P.L.hT_enc0, X, ln);
        store_act16<4>(eacc, X, ln);  // gradient w.r.t. the encoded inputs, slot order (its 0..12), where store_act puts it
      } else {
        f32x16 eacc[4];
        zero_acc<4>(eacc);
#pragma unroll 1
        for (int l = P.num_layers - 1; l >= 1; --l) {
          if (l == P.skip_layer) sweep_gemm<MODE, 4>(eacc, pk + P.L.wT_enc_skip, pk + P.L.hT_enc_skip, X, NB * 4, ln);
          const ReluBits<NB> mb = load_relu_bits<NB>(bits_at(l - 1));
          __builtin_amdgcn_sched_barrier(0);
          f32x16 acc[NB];
          zero_acc<NB>(acc);
          sweep_gemm<MODE, NB>(acc, pk + P.L.wT_x[l], pk + P.L.hT_x[l], X, NB * 4, ln);
          store_masked_bits<NB>(acc, X, mb, h);
        }
        sweep_gemm<MODE, 4>(eacc, pk + P.L.wT_enc0, pk + P.L.hT_enc0, X, NB * 4, ln);
        store_act<4, 4, false>(eacc, X);  // gradient w.r.t. this lane's encoded inputs, slot order (its 0..12)
      }
      float nrm[3];
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const float x = (c == 0) ? mc[0] : (c == 1 ? mc[1] : mc[2]);
        const float v = (c == 0) ? vc[0] : (c == 1 ? vc[1] : vc[2]);
        const float sx = 6.283185307179586f * x;
        float part = 0.0f;
#pragma unroll 2
        for (int jj = 0; jj < 8; ++jj) {
          const float f = h ? P.freqs[8 + jj] : P.freqs[jj];
          const float ang = sx * f;
          const float e = has_cov ? expf(-0.5f * (v * (f * f))) : 1.0f;
          const int u = c * 8 + jj;
          const float gs = Xf[(u >> 2) * 256 + (u & 3)];
          const float gc = Xf[((u + 24) >> 2) * 256 + ((u + 24) & 3)];
          part += (gs * (e * cos_big(ang)) + gc * (e * cos_big(ang + 1.5707963267948966f))) * f;
        }
        part *= 6.283185307179586f;
        if (h == 0) part += Xf[12 * 256 + c];  // the raw-coordinate input column
        const float tot = part + __shfl_xor(part, 32, 64);
        if (c == 0) nrm[0] = tot; else if (c == 1) nrm[1] = tot; else nrm[2] = tot;
      }
      if (h == 0 && valid) {
        const float len = fmaxf(sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]), 1e-12f);
        a.saved.normals[pc * 3 + 0] = -(nrm[0] / len);
        a.saved.normals[pc * 3 + 1] = -(nrm[1] / len);
        a.saved.normals[pc * 3 + 2] = -(nrm[2] / len);
      }
    }
  }
}
