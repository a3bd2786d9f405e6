// rsn_gemm_loops.h -- the per-wave MFMA K loops of the forward (rsn_field_kernel.h) and backward (rsn_field_bwd.hip) field kernels
// over packed weight segments, with what they load and store through (weight-fragment buffer loads, the saved-row buffer stores, the
// bf16 splits) and what an rsn_mma_mode means to them (MmaTraits).  The accumulator <-> LDS-slab epilogues are rsn_epilogues.h.
// See rsn_field.hip for the layout argument (why activations never cross lanes).
#pragma once
#include "rsn_device_math.h"

// Rows kept for the backward pass / the weight gradients.  fp32 rows in the exact and the split-bf16 modes; in the
// reduced-precision training mode (RSN_MMA_BF16: the GEMMs round these values to bf16 anyway) the wide buffers
// (activations, bottleneck, mid hidden; layer gradients) are stored AS bf16 -- half the step's HBM stream.  `save`
// stays a float* in the signatures; SBF reinterprets it as a row of bf16 (element offsets, not bytes).
template <bool SBF>
__device__ __forceinline__ void put4(float* save, int off, const float4 v) {
  if (SBF) {
    const bf16x4 o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
    *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(save) + off) = o;
  } else {
    *reinterpret_cast<float4*>(save + off) = v;
  }
}

// The same rows through BUFFER stores (the product kernels): the descriptor covers the tile's VALID rows of a row-major
// [N, row_elems] buffer (base = the tile's first row, wave-uniform), the lane sends one 32-bit offset (its row + 16 h
// bytes) and the (block, q) position is a scalar offset.  Lanes past the last valid row fall outside the descriptor's
// range and the hardware drops their stores: no per-lane null pointers, no exec-masked branches around the stores.
// cache policy of the saved-row buffer stores (aux bits: 0 = default, 2 = nt): the default policy measured best for the
// per-wave-stream kernels in round 3 (the LDS-ring training kernels use nt, rsn_ringt.h)
#define RSN_SAVED_ROW_AUX 0
struct RowBuf {
  __amdgpu_buffer_rsrc_t r;
  unsigned voff;
  unsigned lim;  // bytes of one row (sv_put_it: K-iterations past the row are not stored)
  bool on;
};
template <bool SBF>
__device__ __forceinline__ RowBuf rowbuf(float* base, long long elem, int rows, int row_elems, int m, int h) {
  constexpr int BPE = SBF ? 2 : 4;
  RowBuf b;
  // a literal nullptr (eval instantiations) removes the stores at compile time; a buffer that is absent at run time gets
  // an empty range instead of a branch around every store
  b.on = !(__builtin_constant_p(base == nullptr) && base == nullptr);
  b.r = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(base) + elem * BPE, 0,
                                          base != nullptr ? rows * row_elems * BPE : 0, 0x00020000);
  b.voff = (unsigned)((m * row_elems + 4 * h) * BPE);
  b.lim = (unsigned)(row_elems * BPE);
  return b;
}
__device__ __forceinline__ bool sv_on(const float* s) { return s != nullptr; }
__device__ __forceinline__ bool sv_on(const RowBuf& b) { return b.on; }
template <bool SBF>
__device__ __forceinline__ void sv_put(float* save, int nb, int q, int h, const float4 v) {
  put4<SBF>(save, (nb * 4 + q) * 8 + 4 * h, v);
}
template <bool SBF>
__device__ __forceinline__ void sv_put(const RowBuf& b, int nb, int q, int, const float4 v) {
  if (SBF) {
    const bf16x4 o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), b.r, b.voff + (unsigned)((nb * 4 + q) * 16), 0, RSN_SAVED_ROW_AUX);
  } else {
    const u32x4 o = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    // (offset in the vector offset / immediate, scalar offset 0: a > 8-byte buffer store with a REGISTER soffset is not protected
    // by hipcc against a VALU overwriting its data registers in the next instruction -- see st16, rsn_ringt.h)
    __builtin_amdgcn_raw_buffer_store_b128(o, b.r, b.voff + (unsigned)((nb * 4 + q) * 32), 0, RSN_SAVED_ROW_AUX);
  }
}
// the float4 of K-iteration `it` of the lane's row (features it*8 + 4h ..): the same bytes sv_put(nb = it/4, q = it%4) writes
__device__ __forceinline__ void sv_put_it(const float*, int, const float4) {}
__device__ __forceinline__ void sv_put_it(const RowBuf& b, int it, const float4 v) {
  const u32x4 o = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  if ((unsigned)it * 32u < b.lim) __builtin_amdgcn_raw_buffer_store_b128(o, b.r, b.voff + (unsigned)it * 32u, 0, RSN_SAVED_ROW_AUX);  // wave-uniform
}

// ------------------------------------------------------------------------------------------------
// MFMA K loop: acc[nb] += W_seg[nb-block] * X, weights double-buffered in registers.
// ------------------------------------------------------------------------------------------------
// NBT = output blocks of the packed segment ([it][NBT][lane][4]); a wave that takes only NBO < NBT of them passes its
// segment pointer already advanced to its first block (tools/probes/gemm_occ_probe.hip).
// Weight fragments arrive through BUFFER loads: the segment base lives in a scalar buffer descriptor, the K-iteration in
// the scalar offset, and a lane sends ONE 32-bit offset (lane * 16 + nb KiB, loop-invariant registers) instead of a
// 64-bit address that a v_add_co pair advances per load.  The 64-bit-address form (global_load_dwordx4 v[lo:hi]) was the
// unexplained per-load cost of rounds 1-2: with buffer loads the eval kernel went 4.90 -> 4.63 ms (83.8 -> 88.6 % of the fp32-MFMA
// peak) and the training forward 22.5 -> 21.4 ms per step (76.6 -> 80.4 %), same box (profiles/r03_buffer_loads.txt).
// Reads past the descriptor's 2 GiB window return 0 (never reached: a packed segment is < 1 MiB).
struct WBuf {
  __amdgpu_buffer_rsrc_t r;
  unsigned voff;  // lane * 16
};
__device__ __forceinline__ WBuf wbuf_make(const float* __restrict__ wseg, int lane) {
  WBuf b;
  b.r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wseg), 0, 0x7fffffff, 0x00020000);
  b.voff = (unsigned)lane * 16u;
  return b;
}
template <int NBO, int NBT = NBO>
__device__ __forceinline__ void load_w(float4 (&w)[NBO], const WBuf& b, int it) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b.r, b.voff + nb * 1024u, (unsigned)it * (NBT * 1024u), 0);
    w[nb] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
}

template <int NBO>
__device__ __forceinline__ void mma4(f32x16 (&acc)[NBO], const float4 (&w)[NBO], const float4 b) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nb].x, b.x, acc[nb], 0, 0, 0);
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nb].y, b.y, acc[nb], 0, 0, 0);
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nb].z, b.z, acc[nb], 0, 0, 0);
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nb].w, b.w, acc[nb], 0, 0, 0);
}

// wseg: packed segment base (global), xl: this lane's slot of the LDS slab (float4 units, stride 64 per it).
// Software pipeline: the loads of K-iteration it+1 are issued while the 32 MFMAs of iteration it run, one load
// after each of the first NBO MFMAs (sched_group_barrier pattern), so every load has a full iteration (2048 MFMA
// cycles) of cover; hipcc on its own sinks the loads to just ahead of their first use.
// Measured with per-phase cycle counters (round 3, BASELINE config 2): with global_load_dwordx4 (64-bit VGPR addresses) the trunk K
// loops ran at 93.5 % of the MFMA issue rate and neither the prefetch distance, the position of the loads nor L1 residency
// changed that; with buffer loads (load_w above) they run at 98.4 % (profiles/r03_phase_eval.json): the cost was the
// address path of the load, not its data or its latency.
template <int NBO>
__device__ __forceinline__ void interleave_loads() {
#pragma unroll
  for (int g = 0; g < NBO; ++g) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // the LDS read of the activations
}

// First weight fragment of a segment: issued by the caller ahead of the epilogue in front of the GEMM so that its L2
// round trip hides under that epilogue.
template <int NBO, int NBT = NBO>
__device__ __forceinline__ void pre_w(float4 (&wa)[NBO], const float* __restrict__ wseg, int lane) {
  load_w<NBO, NBT>(wa, wbuf_make(wseg, lane), 0);
}

// `save` (optional): the rows of the activations this GEMM READS are kept for the backward pass (rsn_field_saved.act /
// bott / hid; rsn_field_grads_out.dy ...).  The K loop holds float4 `it` of the lane's row in a register anyway (the
// MFMA B operand), so the row leaves as ONE buffer store per K-iteration, 2,048 MFMA cycles apart -- instead of a burst
// of 32 stores in the epilogue that produced it, which blocked the wave at the CU's 64 B/clk write port
// (profiles/r03_store_in_loop.txt).
// PF2: the weight fragments TWO K-iterations ahead (three fragment buffers, 4,096 MFMA cycles of cover).  The training
// kernels stream forward AND transposed weights, 4.5 MB against the 4 MiB L2 of an XCD, so part of their stream comes from
// beyond the L2 and one iteration of cover is short: training forward 20.9 -> 20.3 ms per step (82.2 -> 84.7 % of the
// fp32-MFMA peak), backward 11.97 -> 11.81 ms.  The eval kernel's 2.5 MB stay in L2 and it is 1 % slower this way (4.64 ->
// 4.70 ms): it keeps the two-buffer loop below.
template <int NBO, int NBT = NBO, class SV = const float*>
__device__ __forceinline__ void gemm_run2(f32x16 (&acc)[NBO], float4 (&wa)[NBO], const float* __restrict__ wseg,
                                           const float4* xl, int n_it, int lane, SV save = nullptr) {
  const WBuf wp = wbuf_make(wseg, lane);
  float4 wb[NBO], wc[NBO];
  float4 b0, b1, b2;
  auto cl = [&](int i) { return i < n_it ? i : n_it - 1; };
  load_w<NBO, NBT>(wb, wp, cl(1));
  b0 = xl[0];
  int it = 0;
#pragma unroll 1
  for (; it + 2 < n_it; it += 3) {
    load_w<NBO, NBT>(wc, wp, cl(it + 2));
    b1 = xl[cl(it + 1) * 64];
    mma4<NBO>(acc, wa, b0);
    if (sv_on(save)) sv_put_it(save, it, b0);
    interleave_loads<NBO>();
    __builtin_amdgcn_sched_barrier(0);
    load_w<NBO, NBT>(wa, wp, cl(it + 3));
    b2 = xl[cl(it + 2) * 64];
    mma4<NBO>(acc, wb, b1);
    if (sv_on(save)) sv_put_it(save, it + 1, b1);
    interleave_loads<NBO>();
    __builtin_amdgcn_sched_barrier(0);
    load_w<NBO, NBT>(wb, wp, cl(it + 4));
    b0 = xl[cl(it + 3) * 64];
    mma4<NBO>(acc, wc, b2);
    if (sv_on(save)) sv_put_it(save, it + 2, b2);
    interleave_loads<NBO>();
    __builtin_amdgcn_sched_barrier(0);
  }
  if (it < n_it) {
    mma4<NBO>(acc, wa, b0);
    if (sv_on(save)) sv_put_it(save, it, b0);
  }
  if (it + 1 < n_it) {
    b1 = xl[(it + 1) * 64];
    mma4<NBO>(acc, wb, b1);
    if (sv_on(save)) sv_put_it(save, it + 1, b1);
  }
}

template <int NBO, int NBT = NBO, class SV = const float*>
__device__ __forceinline__ void gemm_run(f32x16 (&acc)[NBO], float4 (&wa)[NBO], const float* __restrict__ wseg,
                                          const float4* xl, int n_it, int lane, SV save = nullptr) {
  const WBuf wp = wbuf_make(wseg, lane);
  float4 wb[NBO];
  float4 ba, bb;
  ba = xl[0];
  int it = 0;
#pragma unroll 1
  for (; it + 1 < n_it; it += 2) {
    load_w<NBO, NBT>(wb, wp, it + 1);
    bb = xl[(it + 1) * 64];
    mma4<NBO>(acc, wa, ba);
    if (sv_on(save)) sv_put_it(save, it, ba);
    interleave_loads<NBO>();
    __builtin_amdgcn_sched_barrier(0);
    {  // unconditional prefetch with a clamped index: one control path => exact vmcnt counts
      const int in = (it + 2 < n_it) ? it + 2 : n_it - 1;
      load_w<NBO, NBT>(wa, wp, in);
      ba = xl[in * 64];
    }
    mma4<NBO>(acc, wb, bb);
    if (sv_on(save)) sv_put_it(save, it + 1, bb);
    interleave_loads<NBO>();
    __builtin_amdgcn_sched_barrier(0);
  }
  if (it < n_it) {
    mma4<NBO>(acc, wa, ba);
    if (sv_on(save)) sv_put_it(save, it, ba);
  }
}

// ------------------------------------------------------------------------------------------------
// Split-bf16 K loop (RSN_MMA_BF16X6 / X3): the same GEMM on v_mfma_f32_32x32x16_bf16.
// One K=16 step consumes the lane's two float4's of LDS iterations 2kk, 2kk+1 (same lane-local activations as
// the fp32 loop).  The 8 fp32 activations are split exactly into bf16 triples in registers; the weights arrive
// pre-split ([k16][nb][split][lane][8 bf16], rsn_pack.hip).  NSPLIT = 3: products w1x1, w1x2, w2x1, w1x3, w2x2,
// w3x1 (dropped terms <= 2^-24 relative);  NSPLIT = 2: w1x1, w1x2, w2x1.
// Weight fragments are double-buffered at half-step granularity (half of the output blocks) to fit the VGPR budget.
// ------------------------------------------------------------------------------------------------
struct BSplit {
  bf16x8 s1, s2, s3;
};

template <int NSPLIT>
__device__ __forceinline__ BSplit split8(const float4 lo, const float4 hi) {
  const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  BSplit o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 b1 = (__bf16)x[e];
    const float r1 = x[e] - (float)b1;
    const __bf16 b2 = (NSPLIT >= 2) ? (__bf16)r1 : (__bf16)0.0f;
    o.s1[e] = b1;
    o.s2[e] = b2;
    if (NSPLIT == 3) {
      const float r2 = r1 - (float)b2;
      o.s3[e] = (__bf16)r2;
    } else {
      o.s3[e] = (__bf16)0.0f;
    }
  }
  return o;
}

template <int NH, int NSPLIT>
__device__ __forceinline__ void load_w16(bf16x8 (&w)[NH][3], const WBuf& wp, int kk, int nbo, int nb0) {
#pragma unroll
  for (int t = 0; t < NH; ++t)
#pragma unroll
    for (int sp = 0; sp < NSPLIT; ++sp) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wp.r, wp.voff, (unsigned)(((kk * nbo + nb0 + t) * 3 + sp) * 1024), 0);
      w[t][sp] = __builtin_bit_cast(bf16x8, v);
    }
}

// FULL (NSPLIT = 3 only): all NINE piece products -- w3x3, w3x2, w2x3 ahead of the six, so that the smallest terms meet the
// accumulator first.  Every piece product is exact in fp32 and the pieces add up to the fp32 operands, so no term of the fp32
// product is dropped: the result differs from the fp32 MFMA's only by the order of the fp32 accumulation.  (The analytic-normal sweep
// ran this form until it moved to the 16x16x32 shape, gemm_bf16_s16 below; tools/probes/sweep_x9_probe.hip still times the two
// side by side.)
template <int NBO, int NH, int NB0, int NSPLIT, bool FULL = false>
__device__ __forceinline__ void mma16(f32x16 (&acc)[NBO], const bf16x8 (&w)[NH][3], const BSplit& b) {
  static_assert(!FULL || NSPLIT == 3, "the full product is over three pieces a side");
#pragma unroll
  for (int t = 0; t < NH; ++t) {
    f32x16 c = acc[NB0 + t];
    if (FULL) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][2], b.s3, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][2], b.s2, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][1], b.s3, c, 0, 0, 0);
    }
    if (NSPLIT == 3) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][2], b.s1, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][1], b.s2, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][0], b.s3, c, 0, 0, 0);
    }
    if (NSPLIT >= 2) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][1], b.s1, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][0], b.s2, c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][0], b.s1, c, 0, 0, 0);
    acc[NB0 + t] = c;
  }
}

template <int NBO, int NSPLIT, bool FULL = false>
__device__ __forceinline__ void gemm_bf16(f32x16 (&acc)[NBO], const float* __restrict__ wseg, const float4* xl,
                                          int n_k16, int lane) {
  constexpr int H0 = (NBO + 1) / 2, H1 = NBO - H0;
  constexpr int PER = FULL ? 9 : (NSPLIT == 3 ? 6 : (NSPLIT == 2 ? 3 : 1));  // MFMAs per output block and K step
  const WBuf wp = wbuf_make(wseg, lane);
  bf16x8 wa[H0][3], wb[H1 > 0 ? H1 : 1][3];
  load_w16<H0, NSPLIT>(wa, wp, 0, NBO, 0);
  BSplit bc = split8<NSPLIT>(xl[0], xl[64]);
  const int k1 = n_k16 > 1 ? 1 : 0;
  float4 xlo = xl[(2 * k1) * 64], xhi = xl[(2 * k1 + 1) * 64];  // fp32 activations of the NEXT K step
#pragma unroll 1
  for (int kk = 0; kk < n_k16; ++kk) {
    // ---- phase A: first-half MFMAs; the 3-way split of the next step's activations rides in their issue gaps
    //      (matrix and vector pipes are separate; one 32-cycle MFMA leaves room for a few single-issue VALU ops)
    if (H1 > 0) load_w16<(H1 > 0 ? H1 : 1), NSPLIT>(wb, wp, kk, NBO, H0);
    __builtin_amdgcn_sched_barrier(0);
    const BSplit bn = split8<NSPLIT>(xlo, xhi);
    mma16<NBO, H0, 0, NSPLIT, FULL>(acc, wa, bc);
#pragma unroll
    for (int g = 0; g < H0 * PER; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // 2 VALU
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- phase B: prefetch (unconditional, clamped: one control path keeps the s_waitcnt counts exact), then the
    //      second-half MFMAs
    const int kn = (kk + 1 < n_k16) ? kk + 1 : kk;
    const int k2 = (kk + 2 < n_k16) ? kk + 2 : kn;
    load_w16<H0, NSPLIT>(wa, wp, kn, NBO, 0);
    xlo = xl[(2 * k2) * 64];
    xhi = xl[(2 * k2 + 1) * 64];
    __builtin_amdgcn_sched_barrier(0);
    if (H1 > 0) mma16<NBO, (H1 > 0 ? H1 : 1), (H1 > 0 ? H0 : 0), NSPLIT, FULL>(acc, wb, bc);
    __builtin_amdgcn_sched_barrier(0);
    bc = bn;
  }
}

// ------------------------------------------------------------------------------------------------
// What an rsn_mma_mode (include/rsn.h) means to the per-wave kernels rsn_field_kernel<NB, TRAIN, MMA> and
// rsn_field_bwd_kernel<NB, MMA>, stated once.  (The template parameter stays an int: the kernels' names carry the number.)
// ------------------------------------------------------------------------------------------------
template <int MMA>
struct MmaTraits {
  // training: the bottleneck folded into mlp_mid (rsn_field_kernel.h).  The folded kernels also read the packed bf16 pieces of their
  // buffer: h_x[l] (the forward trunk's W x W GEMMs), hT_seed / hT_x / hT_enc* (the normal sweep), hT_last / hT_x (the backward sweep)
  static constexpr bool FOLD = MMA == RSN_MMA_F32_FOLDED;
  static constexpr int LOOPS = FOLD ? RSN_MMA_F32 : MMA;   // the arithmetic of the K loops: the folded kernels run the exact-fp32 ones
  static constexpr bool F32 = LOOPS == RSN_MMA_F32;        // fp32 MFMA over K-iterations of 8; else (split) bf16 over K = 16 steps
  static constexpr int NSPLIT = LOOPS == RSN_MMA_BF16X6 ? 3 : (LOOPS == RSN_MMA_BF16X3 ? 2 : 1);  // bf16 pieces per operand
  static constexpr bool SAVE_BF16 = LOOPS == RSN_MMA_BF16;  // training: the wide saved rows are stored as bf16 (put4)
  // training: a saved row leaves from the K loop of the GEMM that READS it (gemm_run's `save`); else from the epilogue that produces it
  static constexpr bool LOOP_STORES = F32;
};

// the first fp32 weight fragment of a GEMM, fetched early by the caller (pre_mode ... gemm_mode_run); the split-bf16 loops fetch
// their own first fragment (pre_mode is a no-op for them)
template <int MODE, int NBO, int NBT = NBO>
__device__ __forceinline__ void pre_mode(float4 (&wa)[NBO], const float* __restrict__ w32, int lane) {
  if constexpr (MmaTraits<MODE>::F32) pre_w<NBO, NBT>(wa, w32, lane);
}

// The K loop of the mode: fp32 MFMA over n_it K-iterations of 8, started from the fragment in `wa`; else split-bf16 over
// ceil(n_it / 2) K = 16 steps (those loops take no saver: their epilogues store).
template <int MODE, int NBO, int NBT = NBO, bool PF2 = false, class SV = const float*>
__device__ __forceinline__ void gemm_mode_run(f32x16 (&acc)[NBO], float4 (&wa)[NBO], const float* __restrict__ w32,
                                              const float* __restrict__ w16, const float4* xl, int n_it, int lane,
                                              SV save = nullptr) {
  using M = MmaTraits<MODE>;
  static_assert(M::F32 || NBT == NBO, "the split-bf16 loops own every output block of their segment");
  if constexpr (!M::F32) gemm_bf16<NBO, M::NSPLIT>(acc, w16, xl, (n_it + 1) / 2, lane);
  else if constexpr (PF2) gemm_run2<NBO, NBT>(acc, wa, w32, xl, n_it, lane, save);
  else gemm_run<NBO, NBT>(acc, wa, w32, xl, n_it, lane, save);
}
// The same, fetching the first fragment itself.  Only the fp32 loops have one: a fragment array that is never written moved the
// register allocation of the split kernels (tools/code_object_identity.py), so those go straight to their loop.
template <int MODE, int NBO, int NBT = NBO, bool PF2 = false, class SV = const float*>
__device__ __forceinline__ void gemm_mode(f32x16 (&acc)[NBO], const float* __restrict__ w32, const float* __restrict__ w16,
                                          const float4* xl, int n_it, int lane, SV save = nullptr) {
  if constexpr (MmaTraits<MODE>::F32) {
    float4 wa[NBO];
    pre_w<NBO, NBT>(wa, w32, lane);
    gemm_mode_run<MODE, NBO, NBT, PF2>(acc, wa, w32, w16, xl, n_it, lane, save);
  } else {
    gemm_bf16<NBO, MmaTraits<MODE>::NSPLIT>(acc, w16, xl, (n_it + 1) / 2, lane);
  }
}
// the exact-fp32 loop by itself (tools/probes)
template <int NBO, int NBT = NBO, bool PF2 = false, class SV = const float*>
__device__ __forceinline__ void gemm(f32x16 (&acc)[NBO], const float* __restrict__ wseg, const float4* xl, int n_it,
                                     int lane, SV save = nullptr) {
  gemm_mode<RSN_MMA_F32, NBO, NBT, PF2>(acc, wseg, nullptr, xl, n_it, lane, save);
}

// ------------------------------------------------------------------------------------------------
// Bits K loop (exact-fp32 training, first GEMM of the analytic-normal sweep): acc += V m with m in {0, 1} given as the
// lane's ReLU bits and V = W^T diag(w_density) pre-split into three bf16 pieces (hT_seed, rsn_pack.hip).  A 0 / 1 operand is
// exact in bf16, the three pieces add up to the fp32 value exactly, every product is exact and the accumulation is fp32:
// three v_mfma_f32_32x32x16_bf16 per block and K = 16 step in place of sixteen v_mfma_f32_32x32x2_f32 on the masked seed.
// ------------------------------------------------------------------------------------------------
// B operand of K = 16 step kk: element e is K-iteration 2kk + (e >> 2), component e & 3 -- bit (kk & 3) * 8 + e of word kk / 4
// (store_act: bit nb * 16 + 4 q + j of a lane is K-iteration 4 nb + q, component j).  The word is picked by selects over
// static register indices (an indexed read would put the words in scratch).
// BITS: the lane's NBO / 2 mask words of the layer, `w` (ReluBits<NBO>, rsn_epilogues.h).
struct SeedWords {
  unsigned w0, w1, w2, w3;
};
template <int NBO, class BITS>
__device__ __forceinline__ SeedWords seed_words(const BITS& m) {
  static_assert(NBO == 2 || NBO == 4 || NBO == 8, "one, two or four mask words");
  SeedWords s = {m.w[0], 0u, 0u, 0u};
  if constexpr (NBO >= 4) s.w1 = m.w[1];
  if constexpr (NBO >= 8) { s.w2 = m.w[2]; s.w3 = m.w[3]; }
  return s;
}
__device__ __forceinline__ bf16x8 bits_bf16x8(const SeedWords m, int kk) {
  const int wi = kk >> 2;
  const unsigned word = wi == 0 ? m.w0 : (wi == 1 ? m.w1 : (wi == 2 ? m.w2 : m.w3));
  const unsigned by = word >> ((kk & 3) * 8);
  u32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j)  // bf16 1.0 = 0x3f80; element 2j in the low half of dword j
    v[j] = (((by >> (2 * j)) & 1u) * 0x3f80u) | (((by >> (2 * j + 1)) & 1u) * 0x3f800000u);
  return __builtin_bit_cast(bf16x8, v);
}

// the three pieces of NH blocks against one B operand: small pieces first, the blocks interleaved
template <int NBO, int NH>
__device__ __forceinline__ void mma16_bits(f32x16 (&acc)[NBO], const bf16x8 (&w)[NH][3], const bf16x8 b, int nb0) {
#pragma unroll
  for (int sp = 2; sp >= 0; --sp)
#pragma unroll
    for (int t = 0; t < NH; ++t) acc[nb0 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t][sp], b, acc[nb0 + t], 0, 0, 0);
}

// K = 32 NBO (the layer's output features), NBO row blocks; fragment buffers of half a K step like gemm_bf16 (a full step
// ahead is 48 fragments = 192 registers beside the 128 accumulator registers: tools/probes/seed_bits_probe.hip measures both)
template <int NBO, class BITS>
__device__ __forceinline__ void gemm_bf16_bits(f32x16 (&acc)[NBO], const float* __restrict__ wseg, const BITS& m, int lane) {
  static_assert(NBO % 2 == 0, "two fragment buffers of NBO / 2 blocks");
  constexpr int NH = NBO / 2, NK = 2 * NBO;
  const WBuf wp = wbuf_make(wseg, lane);
  bf16x8 wa[NH][3], wb[NH][3];
  load_w16<NH, 3>(wa, wp, 0, NBO, 0);
  const SeedWords mw = seed_words<NBO>(m);
  bf16x8 bc = bits_bf16x8(mw, 0);
#pragma unroll 1
  for (int kk = 0; kk < NK; ++kk) {
    load_w16<NH, 3>(wb, wp, kk, NBO, NH);
    __builtin_amdgcn_sched_barrier(0);
    const int kn = (kk + 1 < NK) ? kk + 1 : kk;  // clamped: one control path keeps the s_waitcnt counts exact
    const bf16x8 bn = bits_bf16x8(mw, kn);   // rides in the issue gaps of the MFMAs below
    mma16_bits<NBO, NH>(acc, wa, bc, 0);
#pragma unroll
    for (int g = 0; g < NH * 3; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // 2 VALU
    }
    __builtin_amdgcn_sched_barrier(0);
    load_w16<NH, 3>(wa, wp, kn, NBO, 0);
    __builtin_amdgcn_sched_barrier(0);
    mma16_bits<NBO, NH>(acc, wb, bc, NH);
    __builtin_amdgcn_sched_barrier(0);
    bc = bn;
  }
}

// The same GEMM without a packed V (RSN_MMA_F32, whose packed buffer carries no seed segment): the three pieces are formed in
// registers from the fp32 fragments of wT_x[L-1] (K-iterations 2kk, 2kk + 1: the eight values of K = 16 step kk) and the density
// row, by the expressions of split_elem (rsn_pack.hip), and meet the accumulators in the order of mma16_bits (lo, mid, hi per
// block): bit for bit the result of gemm_bf16_bits.  About 50 VALU instructions per block and K step against three MFMAs: the
// loop is VALU-bound, but still well under the fp32-MFMA form it replaces (tools/probes/seed_bits_probe.hip).
template <int NBO, int NH>
__device__ __forceinline__ void load_w32_pair(float4 (&f)[NH][2], const WBuf& b, int kk, int nb0) {
#pragma unroll
  for (int t = 0; t < NH; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b.r, b.voff + (unsigned)(nb0 + t) * 1024u, (unsigned)(2 * kk + j) * (NBO * 1024u), 0);
      f[t][j] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
}

template <int NBO, int NH>
__device__ __forceinline__ void mma16_bits_f32(f32x16 (&acc)[NBO], const float4 (&f)[NH][2], const float4 dlo, const float4 dhi,
                                               const bf16x8 b, int nb0) {
#pragma unroll
  for (int t = 0; t < NH; ++t) {
    const float v[8] = {rsn_seed_product(f[t][0].x, dlo.x), rsn_seed_product(f[t][0].y, dlo.y), rsn_seed_product(f[t][0].z, dlo.z),
                        rsn_seed_product(f[t][0].w, dlo.w), rsn_seed_product(f[t][1].x, dhi.x), rsn_seed_product(f[t][1].y, dhi.y),
                        rsn_seed_product(f[t][1].z, dhi.z), rsn_seed_product(f[t][1].w, dhi.w)};
    bf16x8 s1, s2, s3;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const __bf16 b1 = (__bf16)v[e];
      const float r1 = v[e] - (float)b1;
      const __bf16 b2 = (__bf16)r1;
      const float r2 = r1 - (float)b2;
      s1[e] = b1; s2[e] = b2; s3[e] = (__bf16)r2;
    }
    f32x16 c = acc[nb0 + t];
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s3, b, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s2, b, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s1, b, c, 0, 0, 0);
    acc[nb0 + t] = c;
  }
}

// w32seg: wT_x[L-1] ([it][NBO][lane][4]); wd: the packed density row (v_density)
template <int NBO, class BITS>
__device__ __forceinline__ void gemm_f32_bits(f32x16 (&acc)[NBO], const float* __restrict__ w32seg, const float* __restrict__ wd,
                                              const BITS& m, int lane) {
  static_assert(NBO % 2 == 0, "two fragment buffers of NBO / 2 blocks");
  constexpr int NH = NBO / 2, NK = 2 * NBO;
  const WBuf wp = wbuf_make(w32seg, lane);
  const float* __restrict__ wdl = wd + 4 * (lane >> 5);
  float4 fa[NH][2], fb[NH][2];
  load_w32_pair<NBO, NH>(fa, wp, 0, 0);
  const SeedWords mw = seed_words<NBO>(m);
  float4 dlo = *reinterpret_cast<const float4*>(wdl), dhi = *reinterpret_cast<const float4*>(wdl + 8);
#pragma unroll 1
  for (int kk = 0; kk < NK; ++kk) {
    load_w32_pair<NBO, NH>(fb, wp, kk, NH);
    const int kn = (kk + 1 < NK) ? kk + 1 : kk;
    const float4 nlo = *reinterpret_cast<const float4*>(wdl + 16 * kn), nhi = *reinterpret_cast<const float4*>(wdl + 16 * kn + 8);
    const bf16x8 bc = bits_bf16x8(mw, kk);
    mma16_bits_f32<NBO, NH>(acc, fa, dlo, dhi, bc, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_w32_pair<NBO, NH>(fa, wp, kn, 0);
    mma16_bits_f32<NBO, NH>(acc, fb, dlo, dhi, bc, NH);
    __builtin_amdgcn_sched_barrier(0);
    dlo = nlo; dhi = nhi;
  }
}

// ------------------------------------------------------------------------------------------------
// The piece-product loops on v_mfma_f32_16x16x32_bf16 (exact-fp32 training: the forward trunk, the analytic-normal sweep, the folded
// backward sweep): the MFMA cycles of mma16 (4 NP of 16 per block and K = 32 against 2 NP of 32) and its arithmetic per accumulator
// (smallest terms first), on the shape at which the chip holds the higher clock under load.
// NP, the products per accumulator and K step, is the caller's choice, stated at every call:
//   9  every product of three pieces a side: no term of the fp32 product is dropped (the forward trunk, whose values and ReLU bits
//      everything else reads; the backward sweep's dX, rsn_field_bwd.hip);
//   6  without the three smallest, w_lo b_lo, w_lo b_mid, w_mid b_lo.  Nearest-rounding pieces are bounded by |mid| <= 2^-8 |x| and
//      |lo| <= 2^-17 |x|, so each of the two larger dropped terms is at most 2^-25 |w b| and the three sum to at most
//      (2 * 2^-25 + 2^-34) |w b|, with both operands at their worst: the rounding of ONE fp32 product, in a sum that is rounded to
//      fp32 at every MFMA (the analytic-normal sweep, from whose sums no sign decision is taken).  The six are products 3 .. 8 of
//      the nine, in the same order.
// The wave's output tile stays 32 points x 32 NBO rows, as NBO x 2 row halves x 2 point halves results of 16 x 16.  Lane L = (i = L & 15, g = L >> 4) owns K group g of a K = 32 step,
// which is K group g & 1 of K = 16 step 2 s + (g >> 1): it reads the 16-byte granule of OLD lane (i + 16 rh) + 32 (g & 1) of the
// very records the 32x32x16 loop reads (no other packing), and the two float4 of old lane (i + 16 ph) + 32 (g & 1) of the X slab,
// so A and B meet on the same K set at every MFMA position and the K permutation of the packing carries over.
// Accumulator register r of result (nb, rh, ph) is row 32 nb + 16 rh + 4 (L >> 4) + r of point i + 16 ph: in the X layout of
// store_act one float4, K-iteration 4 nb + 2 rh + (L >> 5) of old lane (i + 16 ph) + 32 ((L >> 4) & 1).
// K must be a multiple of 32 (the kernels pad their widths to 32): no tail path.
// ------------------------------------------------------------------------------------------------
// the lane's place in the 16-shape: the old lane whose operand granules it reads for row half / point half 0 (the other half is
// 16 old lanes on), and the half K = 32 step it owns
struct Lane16 {
  int ol;  // (L & 15) + 32 ((L >> 4) & 1)
  int kh;  // L >> 5
};
__device__ __forceinline__ Lane16 lane16(int lane) {
  Lane16 g;
  g.ol = (lane & 15) + 2 * (lane & 16);
  g.kh = lane >> 5;
  return g;
}

// the last NP of the nine products of NQ blocks against the two point halves, in mma16<.., true>'s order per accumulator; the four
// results of a block take each product in turn (four independent accumulators between two MFMAs of one chain)
__device__ __forceinline__ bf16x8 piece(const BSplit& b, int k) { return k == 0 ? b.s1 : (k == 1 ? b.s2 : b.s3); }  // k: a constant
constexpr int prod_wp(int p) { constexpr int t[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0}; return t[p]; }  // product p: the weight's piece
constexpr int prod_bp(int p) { constexpr int t[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0}; return t[p]; }  //            the activation's piece
template <int NBO, int NQ, int NP>
__device__ __forceinline__ void mma16s(f32x4 (&acc)[NBO][2][2], const bf16x8 (&w)[NQ][2][3], const BSplit (&b)[2], int nb0) {
  static_assert(NP == 9 || NP == 6, "all nine piece products, or the six without w_lo b_lo, w_lo b_mid, w_mid b_lo");
#pragma unroll
  for (int t = 0; t < NQ; ++t)
#pragma unroll
    for (int p = 9 - NP; p < 9; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[nb0 + t][q >> 1][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t][q >> 1][prod_wp(p)], piece(b[q & 1], prod_bp(p)),
                                                                              acc[nb0 + t][q >> 1][q & 1], 0, 0, 0);
}

// the packed pieces of NQ blocks (both row halves) of K = 32 step s; wp.voff carries the lane's granule (gemm_bf16_s16)
template <int NQ>
__device__ __forceinline__ void load_w16s(bf16x8 (&w)[NQ][2][3], const WBuf& wp, int s, int nbo, int nb0) {
#pragma unroll
  for (int t = 0; t < NQ; ++t)
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int sp = 0; sp < 3; ++sp) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wp.r, wp.voff + rh * 256u, (unsigned)(((2 * s * nbo + nb0 + t) * 3 + sp) * 1024), 0);
        w[t][rh][sp] = __builtin_bit_cast(bf16x8, v);
      }
}

// The saved rows of the 16-shape (gemm_run2's `save`, see there): the two float4 a lane reads of old lane ol + 16 ph, K-iterations
// `it` and it + 1 of that point's row.  `b` is rowbuf(.., m = L & 15, h = (L >> 4) & 1): the row of point half 1 lies 16 rows on.
// `it` differs between the lanes (kh), so what must not be stored (K-iterations past the row, `live` off) gets an offset outside the
// descriptor's range, where the hardware drops it, instead of a branch: one control path.  Offsets in the vector offset only.
__device__ __forceinline__ void sv_put16(const float*, int, int, bool, const float4, const float4) {}
__device__ __forceinline__ void sv_put16(const RowBuf& b, int it, int ph, bool live, const float4 lo, const float4 hi) {
  const unsigned at = b.voff + (unsigned)ph * 16u * b.lim + (unsigned)it * 32u;
  const unsigned o0 = (live && (unsigned)it * 32u < b.lim) ? at : 0x80000000u;
  const unsigned o1 = (live && (unsigned)it * 32u + 32u < b.lim) ? at + 32u : 0x80000000u;
  const u32x4 v0 = {__float_as_uint(lo.x), __float_as_uint(lo.y), __float_as_uint(lo.z), __float_as_uint(lo.w)};
  const u32x4 v1 = {__float_as_uint(hi.x), __float_as_uint(hi.y), __float_as_uint(hi.z), __float_as_uint(hi.w)};
  __builtin_amdgcn_raw_buffer_store_b128(v0, b.r, o0, 0, RSN_SAVED_ROW_AUX);
  __builtin_amdgcn_raw_buffer_store_b128(v1, b.r, o1, 0, RSN_SAVED_ROW_AUX);
}

// Packed pieces (hT_* segment, [k16][NBO][piece][lane][8 bf16]).  Fragment buffers of a quarter of the blocks (the 96 registers of
// gemm_bf16's two half-step buffers); the next step's activations are split under the first two chunks' MFMAs, one point half each.
// `save` (optional: the backward sweep, the training forward's trunk): every float4 of the slab this GEMM reads leaves once for its saved row -- step 0's ahead of
// the loop, step s + 1's from the registers that are split under the chunks 0 and 1 of step s (two stores a chunk, behind that
// chunk's fragment loads in the vmcnt order).
template <int NBO, int NP, class SV = const float*>
__device__ __forceinline__ void gemm_bf16_s16(f32x4 (&acc)[NBO][2][2], const float* __restrict__ wseg, const float4* xl, int n_k32,
                                              int lane, SV save = nullptr) {
  static_assert(NBO % 2 == 0, "an even number of fragment buffers' worth of blocks");
  constexpr int NQ = NBO >= 4 ? NBO / 4 : 1, NC = NBO / NQ;  // blocks per fragment buffer, chunks per K step (even)
  const Lane16 g = lane16(lane);
  WBuf wp = wbuf_make(wseg, lane);
  wp.voff = (unsigned)g.ol * 16u + (unsigned)g.kh * (NBO * 3072u);
  const float4* xb = xl - lane + g.ol + g.kh * 128;  // LDS iterations 4 s + 2 kh, + 1; point half 1 is 16 float4 on
  bf16x8 wa[NQ][2][3], wb[NQ][2][3];
  load_w16s<NQ>(wa, wp, 0, NBO, 0);
  BSplit bc[2];
  if (sv_on(save)) {  // step 0's four float4, kept for their rows
    const float4 p0lo = xb[0], p0hi = xb[64], p1lo = xb[16], p1hi = xb[80];
    bc[0] = split8<3>(p0lo, p0hi);
    bc[1] = split8<3>(p1lo, p1hi);
    sv_put16(save, 2 * g.kh, 0, true, p0lo, p0hi);
    sv_put16(save, 2 * g.kh, 1, true, p1lo, p1hi);
  } else {
    bc[0] = split8<3>(xb[0], xb[64]);
    bc[1] = split8<3>(xb[16], xb[80]);
  }
  const int s1 = n_k32 > 1 ? 1 : 0;
  float4 x0lo = xb[4 * s1 * 64], x0hi = xb[(4 * s1 + 1) * 64], x1lo = xb[4 * s1 * 64 + 16], x1hi = xb[(4 * s1 + 1) * 64 + 16];
#pragma unroll 1
  for (int s = 0; s < n_k32; ++s) {
    const int sn = (s + 1 < n_k32) ? s + 1 : s;  // clamped: one control path keeps the s_waitcnt counts exact
    const int s2 = (s + 2 < n_k32) ? s + 2 : sn;
    BSplit bn[2];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c & 1) load_w16s<NQ>(wa, wp, c + 1 < NC ? s : sn, NBO, c + 1 < NC ? (c + 1) * NQ : 0);
      else load_w16s<NQ>(wb, wp, s, NBO, (c + 1) * NQ);
      __builtin_amdgcn_sched_barrier(0);
      if (c == 0) bn[0] = split8<3>(x0lo, x0hi);
      if (c == 1) bn[1] = split8<3>(x1lo, x1hi);
      // the registers hold step sn; in the last step that is this step again (the clamp), whose rows have left: not live
      if (c == 0 && sv_on(save)) sv_put16(save, 4 * sn + 2 * g.kh, 0, s + 1 < n_k32, x0lo, x0hi);
      if (c == 1 && sv_on(save)) sv_put16(save, 4 * sn + 2 * g.kh, 1, s + 1 < n_k32, x1lo, x1hi);
      if (c == NC - 1) {
        x0lo = xb[4 * s2 * 64]; x0hi = xb[(4 * s2 + 1) * 64];
        x1lo = xb[4 * s2 * 64 + 16]; x1hi = xb[(4 * s2 + 1) * 64 + 16];
      }
      if (c & 1) mma16s<NBO, NQ, NP>(acc, wb, bc, c * NQ); else mma16s<NBO, NQ, NP>(acc, wa, bc, c * NQ);
#pragma unroll
      for (int m = 0; m < NQ * 4 * NP; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        if (c < 2) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // the next step's pieces: an MFMA leaves 8 of its 16 cycles
        if (c < 2 && sv_on(save) && (m == 8 || m == 20)) __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);  // 1 row store
      }
      if (c == NC - 1) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // the LDS reads of the activations
      __builtin_amdgcn_sched_barrier(0);
    }
    bc[0] = bn[0];
    bc[1] = bn[1];
  }
}

// The same loop without packed pieces (RSN_MMA_F32): the weight pieces formed in registers by split8<3> from the fp32 fragments of
// a wT_* segment ([it][NBO][lane][4]; the lane reads K-iterations 4 s + 2 kh, + 1 of old lane ol + 16 rh), the same NP products in
// the same order per accumulator: bit for bit the packed form.  A software pipeline over the 2 NBO row halves of a K step: the pieces
// of row half u + 1 are formed under the 2 NP MFMAs of row half u (the last two also split the next step's activations).  A
// 16-cycle MFMA leaves the VALU 8 cycles where a 32-cycle one left 24, so about 50 VALU instructions per 18 MFMAs (12 at NP = 6,
// which therefore gains nothing here) make this loop VALU-bound: it takes 1.01-1.03 of the time of its 32x32x16 form (tools/probes/sweep_x9_probe.hip, forms (e) and (c)) and the
// unfolded primary forward launch 3 % more (profiles/normals_shape16.json); it is on this shape for the bits it shares with the
// packed loop.  A fragment buffer (a quarter of the blocks) is dead once its last row half is split and is reloaded, two
// chunks ahead, under the MFMAs of that row half.
template <int NQ>
__device__ __forceinline__ void load_w32s(float4 (&f)[NQ][2][2], const WBuf& b, int s, int nbo, int nb0) {
#pragma unroll
  for (int t = 0; t < NQ; ++t)
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b.r, b.voff + rh * 256u, (unsigned)(((4 * s + j) * nbo + nb0 + t) * 1024), 0);
        f[t][rh][j] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
      }
}

// `save` (optional): as in gemm_bf16_s16 -- step 0's float4 ahead of the loop, step s + 1's from the registers that the last two row
// halves of step s split.
template <int NBO, int NP, class SV = const float*>
__device__ __forceinline__ void gemm_f32_s16(f32x4 (&acc)[NBO][2][2], const float* __restrict__ w32seg, const float4* xl,
                                                int n_k32, int lane, SV save = nullptr) {
  static_assert(NBO % 2 == 0, "an even number of fragment buffers' worth of blocks");
  static_assert(NP == 9 || NP == 6, "all nine piece products, or the six without w_lo b_lo, w_lo b_mid, w_mid b_lo");
  constexpr int NQ = NBO >= 4 ? NBO / 4 : 1, NC = NBO / NQ, UQ = 2 * NQ, NU = 2 * NBO;  // row halves per chunk and per K step
  // per MFMA of a row half: the VALU instructions scheduled behind it, and the two MFMAs that a row store follows.  At nine
  // products the requests place 3 x 18 = 54 / 6 x 18 = 108 VALU instructions a row half, all of the split's.  At six they place
  // 2 x 12 = 24 / 4 x 12 = 48, fewer than half; the rest go where hipcc puts them.  Larger groups at six (4 / 8 and up) crash hipcc
  // (ROCm 7.2, clang 22: a segmentation fault in its AGPR-copy-MFMA rewrite pass on rsn_field_kernel<8, true, 0>).  The loop is
  // VALU-bound either way.
  constexpr int VA = NP == 9 ? 3 : 2, VB = NP == 9 ? 6 : 4, ST0 = NP == 9 ? 5 : 3, ST1 = NP == 9 ? 12 : 8;
  const Lane16 g = lane16(lane);
  WBuf wp = wbuf_make(w32seg, lane);
  wp.voff = (unsigned)g.ol * 16u + (unsigned)g.kh * (NBO * 2048u);
  const float4* xb = xl - lane + g.ol + g.kh * 128;
  float4 fa[NQ][2][2], fb[NQ][2][2];
  load_w32s<NQ>(fa, wp, 0, NBO, 0);
  load_w32s<NQ>(fb, wp, 0, NBO, NQ);
  BSplit bc[2];
  if (sv_on(save)) {  // step 0's four float4, kept for their rows
    const float4 p0lo = xb[0], p0hi = xb[64], p1lo = xb[16], p1hi = xb[80];
    bc[0] = split8<3>(p0lo, p0hi);
    bc[1] = split8<3>(p1lo, p1hi);
    sv_put16(save, 2 * g.kh, 0, true, p0lo, p0hi);
    sv_put16(save, 2 * g.kh, 1, true, p1lo, p1hi);
  } else {
    bc[0] = split8<3>(xb[0], xb[64]);
    bc[1] = split8<3>(xb[16], xb[80]);
  }
  const int s1 = n_k32 > 1 ? 1 : 0;
  float4 x0lo = xb[4 * s1 * 64], x0hi = xb[(4 * s1 + 1) * 64], x1lo = xb[4 * s1 * 64 + 16], x1hi = xb[(4 * s1 + 1) * 64 + 16];
  BSplit w = split8<3>(fa[0][0][0], fa[0][0][1]);
  BSplit bn[2] = {bc[0], bc[1]};
#pragma unroll 1
  for (int s = 0; s < n_k32; ++s) {
    const int sn = (s + 1 < n_k32) ? s + 1 : s;  // clamped: one control path keeps the s_waitcnt counts exact
    const int s2 = (s + 2 < n_k32) ? s + 2 : sn;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int un = (u + 1) % NU, cn = (un / UQ) & 1, tn = (un / 2) % NQ;  // the next row half: its buffer and block in it
      const BSplit wn = cn ? split8<3>(fb[tn][un & 1][0], fb[tn][un & 1][1]) : split8<3>(fa[tn][un & 1][0], fa[tn][un & 1][1]);
      const bool reload = u % UQ == UQ - 1;
      if (reload) {
        const int c = u / UQ, c2 = (c + 2) % NC;
        if (c & 1) load_w32s<NQ>(fb, wp, c + 2 < NC ? s : sn, NBO, c2 * NQ);
        else load_w32s<NQ>(fa, wp, c + 2 < NC ? s : sn, NBO, c2 * NQ);
      }
      if (u == NU - 2) bn[0] = split8<3>(x0lo, x0hi);
      // the registers hold step sn; in the last step that is this step again (the clamp), whose rows have left: not live
      if (u == NU - 2 && sv_on(save)) sv_put16(save, 4 * sn + 2 * g.kh, 0, s + 1 < n_k32, x0lo, x0hi);
      if (u == NU - 1 && sv_on(save)) sv_put16(save, 4 * sn + 2 * g.kh, 1, s + 1 < n_k32, x1lo, x1hi);
      if (u == NU - 1) {
        bn[1] = split8<3>(x1lo, x1hi);
        x0lo = xb[4 * s2 * 64]; x0hi = xb[(4 * s2 + 1) * 64];
        x1lo = xb[4 * s2 * 64 + 16]; x1hi = xb[(4 * s2 + 1) * 64 + 16];
      }
#pragma unroll
      for (int p = 9 - NP; p < 9; ++p)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
          acc[u >> 1][u & 1][ph] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(piece(w, prod_wp(p)), piece(bc[ph], prod_bp(p)),
                                                                           acc[u >> 1][u & 1][ph], 0, 0, 0);
#pragma unroll
      for (int m = 0; m < 2 * NP; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        if (reload && m < NQ * 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
        if (u >= NU - 2) __builtin_amdgcn_sched_group_barrier(0x002, VB, 0);  // the next row half's pieces + the next step's activations
        else __builtin_amdgcn_sched_group_barrier(0x002, VA, 0);  // the next row half's pieces
        if (u >= NU - 2 && sv_on(save) && (m == ST0 || m == ST1)) __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);  // 1 row store
      }
      if (u == NU - 1) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // the LDS reads of the activations
      __builtin_amdgcn_sched_barrier(0);
      w = wn;
    }
    bc[0] = bn[0];
    bc[1] = bn[1];
  }
}

