// rsn_epilogues.h -- the accumulator epilogues of the per-wave field kernels (rsn_field_kernel.h, rsn_field_bwd.hip): how the
// accumulators of one GEMM start (bias / zero) and how they leave for the wave's LDS slab X, where they are the B operand of the next
// GEMM (rsn_gemm_loops.h), for the saved rows and for the ReLU bit masks.  See rsn_field.hip for the layout argument.
#pragma once
#include "rsn_gemm_loops.h"

// acc[nb][4q+j] = bias[nb*32 + 8q + 4h + j]: the accumulators start from the bias (what torch's addmm does),
// so the 4*NBO bias loads are issued back to back ahead of the K loop and the epilogue needs no memory reads.
template <int NBO>
__device__ __forceinline__ void init_acc(f32x16 (&acc)[NBO], const float* __restrict__ bias, int h) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + nb * 32 + 8 * q + 4 * h);
      acc[nb][4 * q + 0] = bv.x;
      acc[nb][4 * q + 1] = bv.y;
      acc[nb][4 * q + 2] = bv.z;
      acc[nb][4 * q + 3] = bv.w;
    }
}

template <int NBO>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NBO]) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.0f;
}

template <int NBO>
__device__ __forceinline__ void zero_acc16(f32x4 (&acc)[NBO][2][2]) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[nb][q >> 1][q & 1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// ReLU sign bits of one lane: bit nb*16 + r = (accumulator register r of block nb, the layer's pre-activation) > 0,
// packed into NBO/2 words (rsn_field_saved.relu_bits).  The dX sweeps mask by these bits instead of re-reading the
// saved fp32 activations (1 KiB per point and layer -> 32 B; 124 fewer live registers in the sweeps).
// The bits of four relu'd values at positions 4 q .. 4 q + 3 (the ReLU epilogues below take the bits from the values they have just
// formed: no second v_max per value).  pre-activation x > 0  <=>  the bits of relu(x) (relu_f: one v_max_i32) are non-zero:
// v_min_u32(., 1), then v_lshl_or_b32.  The C forms (`t > 0`, clamp(t, 0, 1)) become v_cmp_lt_i32 (SGPR pair) + a hazard nop +
// v_cndmask + v_or3.  The asm takes the relu'd value, NOT the accumulator: an asm operand that is an MFMA result is invisible to
// the compiler's hazard recogniser (see relu_f); behind the compiler's own v_max_i32 it is an ordinary VALU result.
template <int Q>
__device__ __forceinline__ unsigned relu_bits4q(unsigned b, const float4 v) {
  const unsigned lo[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    unsigned bit, nb;
    if (Q == 0 && t == 0) {
      asm("v_min_u32 %0, %1, 1" : "=v"(bit) : "v"(lo[t]));
      b = bit;
    } else if (t == 0) {
      asm("v_min_u32 %0, %2, 1\n\tv_lshl_or_b32 %1, %0, %3, %4" : "=&v"(bit), "=v"(nb) : "v"(lo[t]), "n"(4 * Q), "v"(b));
      b = nb;
    } else if (t == 1) {
      asm("v_min_u32 %0, %2, 1\n\tv_lshl_or_b32 %1, %0, %3, %4" : "=&v"(bit), "=v"(nb) : "v"(lo[t]), "n"(4 * Q + 1), "v"(b));
      b = nb;
    } else if (t == 2) {
      asm("v_min_u32 %0, %2, 1\n\tv_lshl_or_b32 %1, %0, %3, %4" : "=&v"(bit), "=v"(nb) : "v"(lo[t]), "n"(4 * Q + 2), "v"(b));
      b = nb;
    } else {
      asm("v_min_u32 %0, %2, 1\n\tv_lshl_or_b32 %1, %0, %3, %4" : "=&v"(bit), "=v"(nb) : "v"(lo[t]), "n"(4 * Q + 3), "v"(b));
      b = nb;
    }
  }
  return b;
}
__device__ __forceinline__ unsigned relu_bits4(unsigned b, const float4 v, int q) {  // q: a constant after unrolling
  return q == 0 ? relu_bits4q<0>(b, v) : (q == 1 ? relu_bits4q<1>(b, v) : (q == 2 ? relu_bits4q<2>(b, v) : relu_bits4q<3>(b, v)));
}

// the lane's NBO/2 mask words of one layer (issued BEFORE the layer's GEMM, consumed by store_masked_bits after it)
template <int NBO>
struct ReluBits {
  unsigned w[NBO / 2];
};

template <int NBO>
__device__ __forceinline__ ReluBits<NBO> load_relu_bits(const unsigned* __restrict__ bits) {
  ReluBits<NBO> m;
  if (NBO >= 8) {
#pragma unroll
    for (int w4 = 0; w4 < NBO / 8; ++w4) {
      const uint4 v = *reinterpret_cast<const uint4*>(bits + w4 * 4);
      m.w[w4 * 4 + 0] = v.x; m.w[w4 * 4 + 1] = v.y; m.w[w4 * 4 + 2] = v.z; m.w[w4 * 4 + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int w = 0; w < NBO / 2; ++w) m.w[w] = bits[w];
  }
  return m;
}

// bit `pos` of `word` as 0 / 0xffffffff: one v_bfe_i32.  Written as (non-volatile) asm because hipcc rewrites
// `x & sext(bit)` into v_and (test) + v_cmp_ne + v_cndmask: three VALU per value and a VCC hazard nop, where bfe + and is two.
__device__ __forceinline__ unsigned bit_mask(int word, int pos) {
  unsigned m;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(word), "n"(pos));
  return m;
}

// dX-sweep epilogue on mask bits: X[it][lane] = bit ? acc : 0 (v_bfe_i32 gives 0 / -1, one v_and applies it);
// optionally also stored to row `save` (backward pass: the layer's pre-activation gradient for the weight gradients)
template <int NBO, bool SBF = false, class SV = float*>
__device__ __forceinline__ void store_masked_bits(const f32x16 (&acc)[NBO], float4* xl, const ReluBits<NBO>& m, int h,
                                                  SV save = nullptr) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int word = m.w[nb / 2];
      const int base = (nb & 1) * 16 + 4 * q;
      float4 v;
      v.x = __uint_as_float(__float_as_uint(acc[nb][4 * q + 0]) & bit_mask(word, base + 0));
      v.y = __uint_as_float(__float_as_uint(acc[nb][4 * q + 1]) & bit_mask(word, base + 1));
      v.z = __uint_as_float(__float_as_uint(acc[nb][4 * q + 2]) & bit_mask(word, base + 2));
      v.w = __uint_as_float(__float_as_uint(acc[nb][4 * q + 3]) & bit_mask(word, base + 3));
      xl[(nb * 4 + q) * 64] = v;
      if (sv_on(save)) sv_put<SBF>(save, nb, q, h, v);
    }
}

// Epilogues of the 16-shape (gemm_bf16_s16, rsn_gemm_loops.h).  One result is one float4 of the X slab; its mask nibble is bits
// 16 nb + 4 (2 rh + kh) .. + 3 of the ReluBits of the old lane that owns that float4, so a lane holds the words of two old lanes
// (point halves 0 and 1).
template <int NBO>
__device__ __forceinline__ void store_masked_bits16(const f32x4 (&acc)[NBO][2][2], float4* xl, const ReluBits<NBO> (&m)[2], int lane) {
  const Lane16 g = lane16(lane);
  float4* xs = xl - lane + g.ol + g.kh * 64;
#pragma unroll
  for (int ph = 0; ph < 2; ++ph)
#pragma unroll
    for (int nb = 0; nb < NBO; ++nb) {
      const int word = (int)(m[ph].w[nb / 2] >> (4 * g.kh));
#pragma unroll
      for (int rh = 0; rh < 2; ++rh) {
        const int base = (nb & 1) * 16 + 8 * rh;
        const f32x4& a = acc[nb][rh][ph];
        float4 v;
        v.x = __uint_as_float(__float_as_uint(a[0]) & bit_mask(word, base + 0));
        v.y = __uint_as_float(__float_as_uint(a[1]) & bit_mask(word, base + 1));
        v.z = __uint_as_float(__float_as_uint(a[2]) & bit_mask(word, base + 2));
        v.w = __uint_as_float(__float_as_uint(a[3]) & bit_mask(word, base + 3));
        xs[(nb * 4 + 2 * rh) * 64 + 16 * ph] = v;
      }
    }
}

template <int NBO>
__device__ __forceinline__ void store_act16(const f32x4 (&acc)[NBO][2][2], float4* xl, int lane) {
  const Lane16 g = lane16(lane);
  float4* xs = xl - lane + g.ol + g.kh * 64;
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4& a = acc[nb][q >> 1][q & 1];
      xs[(nb * 4 + 2 * (q >> 1)) * 64 + 16 * (q & 1)] = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// The training forward's trunk on the 16-shape (exact fp32, rsn_field_kernel.h).  Bias start: register r of result (nb, rh, ph) is
// row 32 nb + 16 rh + 4 (L >> 4) + r, the same for both point halves.
template <int NBO>
__device__ __forceinline__ void init_acc16(f32x4 (&acc)[NBO][2][2], const float* __restrict__ bias, int lane) {
  const float* __restrict__ bl = bias + 4 * (lane >> 4);
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int rh = 0; rh < 2; ++rh) {
      const float4 bv = *reinterpret_cast<const float4*>(bl + nb * 32 + 16 * rh);
      acc[nb][rh][0] = acc[nb][rh][1] = f32x4{bv.x, bv.y, bv.z, bv.w};
    }
}

// ReLU epilogue of the 16-shape: store_act16 of the relu'd values, and the layer's mask words in ReluBits' layout.  The nibble of
// result (nb, rh, ph) is bits 16 (nb & 1) + 4 (2 rh + kh) .. + 3 of word nb / 2 of old lane (L & 15) + 16 ph + 32 ((L >> 4) & 1):
// lanes L and L ^ 32 hold the alternate nibbles (kh = 0 / 1) of the same words.  Each lane collects its nibbles per point half
// (relu_bits4 at q = 2 rh, then shifted by 4 kh), hands the half it does not store to its partner (one 32-lane exchange per word)
// and stores the words of point half kh: `bits` is that old lane's slot, (point (L & 15) + 16 kh, half (L >> 4) & 1), or nullptr.
// REINIT: block by block the accumulators restart from the next layer's bias (init_acc16), like store_act_init.
template <int NBO, bool REINIT>
__device__ __forceinline__ void store_act16_relu_body(f32x4 (&acc)[NBO][2][2], float4* xl, int lane, const float* __restrict__ bias,
                                                      unsigned* bits) {
  static_assert(NBO % 2 == 0, "whole mask words");
  const Lane16 g = lane16(lane);
  float4* xs = xl - lane + g.ol + g.kh * 64;
  const float* __restrict__ bl = bias + 4 * (lane >> 4);
  unsigned bw[2][NBO / 2];
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb) {
    unsigned b16[2] = {0u, 0u};
#pragma unroll
    for (int rh = 0; rh < 2; ++rh) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const f32x4& a = acc[nb][rh][ph];
        const float4 v = make_float4(relu_f(a[0]), relu_f(a[1]), relu_f(a[2]), relu_f(a[3]));
        b16[ph] = relu_bits4(b16[ph], v, 2 * rh);
        xs[(nb * 4 + 2 * rh) * 64 + 16 * ph] = v;
      }
      if constexpr (REINIT) {
        const float4 bv = *reinterpret_cast<const float4*>(bl + nb * 32 + 16 * rh);
        acc[nb][rh][0] = acc[nb][rh][1] = f32x4{bv.x, bv.y, bv.z, bv.w};
      }
    }
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      if (nb & 1) bw[ph][nb / 2] |= b16[ph] << 16; else bw[ph][nb / 2] = b16[ph];
    }
  }
  unsigned ow[NBO / 2];
#pragma unroll
  for (int w = 0; w < NBO / 2; ++w) {
    const unsigned keep = (g.kh ? bw[1][w] : bw[0][w]) << (4 * g.kh);
    const unsigned give = (g.kh ? bw[0][w] : bw[1][w]) << (4 * g.kh);
    ow[w] = keep | (unsigned)__shfl_xor((int)give, 32, 64);
  }
  if (bits) {
    if (NBO >= 8) {
#pragma unroll
      for (int w4 = 0; w4 < NBO / 8; ++w4)
        *reinterpret_cast<uint4*>(bits + w4 * 4) = make_uint4(ow[w4 * 4], ow[w4 * 4 + 1], ow[w4 * 4 + 2], ow[w4 * 4 + 3]);
    } else {
#pragma unroll
      for (int w = 0; w < NBO / 2; ++w) bits[w] = ow[w];
    }
  }
}
template <int NBO>
__device__ __forceinline__ void store_act16_relu(f32x4 (&acc)[NBO][2][2], float4* xl, int lane, unsigned* bits) {
  store_act16_relu_body<NBO, false>(acc, xl, lane, nullptr, bits);
}
template <int NBO>
__device__ __forceinline__ void store_act16_relu_init(f32x4 (&acc)[NBO][2][2], float4* xl, int lane, const float* __restrict__ bias,
                                                      unsigned* bits) {
  store_act16_relu_body<NBO, true>(acc, xl, lane, bias, bits);
}

// the accumulators of the fp32 loop back from the slab: the inverse of store_act without activation (the lane's own float4)
template <int NBO>
__device__ __forceinline__ void load_acc(f32x16 (&acc)[NBO], const float4* xl) {
#pragma unroll
  for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = xl[(nb * 4 + q) * 64];
      acc[nb][4 * q + 0] = v.x;
      acc[nb][4 * q + 1] = v.y;
      acc[nb][4 * q + 2] = v.z;
      acc[nb][4 * q + 3] = v.w;
    }
}

// X[it = nb*4+q][lane] = act(acc[nb][4q..4q+3])   (bias already inside acc, see init_acc).
// save (training): the same float4 also goes to row `save` of a row-major [N, 32*NBS] activation buffer
// (this lane's point; the four q of one nb complete one 128-B line per row).
// REINIT: block by block the accumulators are read out and immediately re-loaded with the next layer's bias (init_acc of the next
// GEMM, same blocks), so the bias round trip hides under the rest of the epilogue.
template <int NBS, bool RELU, bool SBF, bool REINIT, class ACC, class SV>
__device__ __forceinline__ void store_act_body(ACC& acc, float4* xl, SV save, int h, const float* __restrict__ bias, unsigned* bits) {
  unsigned bw[NBS / 2 > 0 ? NBS / 2 : 1];
#pragma unroll
  for (int nb = 0; nb < NBS; ++nb) {
    unsigned b16 = 0u;  // the block's 16 mask bits, taken from the relu'd values as they are formed (dead code without `bits`)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 v = make_float4(acc[nb][4 * q + 0], acc[nb][4 * q + 1], acc[nb][4 * q + 2], acc[nb][4 * q + 3]);
      if (RELU) {
        v.x = relu_f(v.x);
        v.y = relu_f(v.y);
        v.z = relu_f(v.z);
        v.w = relu_f(v.w);
        b16 = relu_bits4(b16, v, q);
      }
      xl[(nb * 4 + q) * 64] = v;
      if (sv_on(save)) sv_put<SBF>(save, nb, q, h, v);
      if constexpr (REINIT) {
        const float4 bv = *reinterpret_cast<const float4*>(bias + nb * 32 + 8 * q + 4 * h);
        acc[nb][4 * q + 0] = bv.x;
        acc[nb][4 * q + 1] = bv.y;
        acc[nb][4 * q + 2] = bv.z;
        acc[nb][4 * q + 3] = bv.w;
      }
    }
    if (RELU) {
      if (nb & 1) bw[nb / 2] |= b16 << 16; else bw[nb / 2] = b16;
    }
  }
  if (RELU && bits) {
    if (NBS >= 8) {
#pragma unroll
      for (int w4 = 0; w4 < NBS / 8; ++w4)
        *reinterpret_cast<uint4*>(bits + w4 * 4) = make_uint4(bw[w4 * 4], bw[w4 * 4 + 1], bw[w4 * 4 + 2], bw[w4 * 4 + 3]);
    } else {
#pragma unroll
      for (int w = 0; w < NBS / 2; ++w) bits[w] = bw[w];
    }
  }
}
// the first NBS blocks of a GEMM's accumulators leave
template <int NBO, int NBS, bool RELU, bool SBF = false, class SV = float*>
__device__ __forceinline__ void store_act(const f32x16 (&acc)[NBO], float4* xl, SV save = nullptr, int h = 0,
                                          unsigned* bits = nullptr) {
  store_act_body<NBS, RELU, SBF, false>(acc, xl, save, h, nullptr, bits);
}
// store_act of one layer fused with init_acc of the next (same NBO)
template <int NBO, bool RELU, bool SBF = false, class SV = float*>
__device__ __forceinline__ void store_act_init(f32x16 (&acc)[NBO], float4* xl, SV save, int h,
                                               const float* __restrict__ bias, unsigned* bits = nullptr) {
  store_act_body<NBO, RELU, SBF, true>(acc, xl, save, h, bias, bits);
}
