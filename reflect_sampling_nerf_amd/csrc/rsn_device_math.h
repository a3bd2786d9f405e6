// rsn_device_math.h -- scalar device maths and the vector typedefs every kernel family shares: no matrix instruction and no buffer
// intrinsic in here.  The per-wave K loops are rsn_gemm_loops.h, the accumulator epilogues rsn_epilogues.h.
#pragma once
#include "rsn_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define RSN_MODE_FRUSTUM 0
#define RSN_MODE_INF 1
#define RSN_MODE_GAUSS 2
#define RSN_MODE_EMB 3

// ------------------------------------------------------------------------------------------------
// small math, written to follow the torch op order of the reference (contraction off: -ffp-contract=off)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// sin / cos of an fp32 argument up to ~1e6 (the IPE reaches 2*pi*2*2^16 = 8.2e5), <= 1.7 ulp -- the quality of ocml's
// sinf (1.57 ulp measured over the same range) at ~1/5 of its instruction count.  Instead of the branchy Payne-Hanek
// path the argument is reduced by multiples of pi/2 with a three-constant Cody-Waite scheme on FUSED multiply-adds:
// pi/2 = C1 + C2 + C3 with C1 = fl32(pi/2); q <= 2^20 is an integer and C1 a multiple of 2^-23, so a - q*C1 is a
// multiple of 2^-23 below 1 in magnitude and the first fma is EXACT; the second rounds once (2^-25), the third term is
// 1e-9.  Reduced argument within 3.1e-8 of the true one (measured over 4e6 arguments up to 8.3e5: max |r| 0.87 --
// the fp32 product a*(2/pi) may pick the neighbouring quadrant, which costs nothing -- and 9.8e-8 / 1.65 ulp on the
// result).  A degree-7/8 minimax pair is evaluated on the reduced argument.  quad = 0: sin, quad = 1: cos.
// Round 1 reduced in fp64 (two v_fma_f64 + five conversions per evaluation): same accuracy, ~2x the issue cycles.
__device__ __forceinline__ float sincos_big(float a, int quad) {
  const float q = rintf(a * 0.63661977236758134308f);
  float r = __builtin_fmaf(-q, 1.5707963705062866f, a);
  r = __builtin_fmaf(-q, -4.371138828673793e-08f, r);
  r = __builtin_fmaf(-q, -1.7151245100058819e-15f, r);
  const int n = (int)q + quad;
  const float s = r * r;
  const float ps = r + r * s * (-1.6666654611e-1f + s * (8.3321608736e-3f + s * (-1.9515295891e-4f)));
  const float pc =
      1.0f + s * (-0.5f + s * (4.166664568298827e-2f + s * (-1.388731625493765e-3f + s * 2.443315711809948e-5f)));
  const float v = (n & 1) ? pc : ps;
  return (n & 2) ? -v : v;
}
__device__ __forceinline__ float sin_big(float a) { return sincos_big(a, 0); }
__device__ __forceinline__ float cos_big(float a) { return sincos_big(a, 1); }

// 34 real-SH polynomial terms, bands l = 1, 2, 4, 8 (reflect_sampling_nerf_components.py:65-127), then the
// per-band roughness attenuation exp(-rho*{1,3,10,36}) (components.py:136-139).
__device__ __forceinline__ void sh34_attenuated(float x, float y, float z, float rho, float sh[34]) {
  const float x2 = x * x, y2 = y * y, z2 = z * z;
  const float xy = x * y, xz = x * z, yz = y * z;
  const float a = x2 - y2;
  const float p = 3.0f * x2 - y2;
  const float q = x2 - 3.0f * y2;
  const float z4 = z2 * z2, x4 = x2 * x2, y4 = y2 * y2;
  const float im5 = y4 - 10.0f * x2 * y2 + 5.0f * x4;
  const float re5 = x4 - 10.0f * x2 * y2 + 5.0f * y4;
  const float im7 = (x2 - 5.0f * y2) * 7.0f * x4 + (21.0f * x2 - y2) * y4;
  const float re7 = (x2 - 21.0f * y2) * x4 + (5.0f * x2 - y2) * 7.0f * y4;
  const float re4 = x2 * q - y2 * p;
  const float t6 = 143.0f * z4 * z2 - 143.0f * z4 + 33.0f * z2 - 1.0f;
  const float t7 = 715.0f * z4 * z2 - 1001.0f * z4 + 385.0f * z2 - 35.0f;
  const float t5 = 39.0f * z4 - 26.0f * z2 + 3.0f;
  const float t4 = 65.0f * z4 - 26.0f * z2 + 1.0f;
  const float e1 = expf(-rho), e2 = expf(-rho * 3.0f), e4 = expf(-rho * 10.0f), e8 = expf(-rho * 36.0f);
  sh[0] = 0.48860251190291992f * y * e1;
  sh[1] = 0.48860251190291992f * z * e1;
  sh[2] = 0.48860251190291992f * x * e1;
  sh[3] = 1.09254843059207907f * xy * e2;
  sh[4] = 1.09254843059207907f * yz * e2;
  sh[5] = 0.31539156525252001f * (3.0f * z2 - 1.0f) * e2;
  sh[6] = 1.09254843059207907f * xz * e2;
  sh[7] = 0.54627421529603953f * a * e2;
  sh[8] = 2.50334294179670453f * xy * a * e4;
  sh[9] = 1.77013076977993053f * yz * p * e4;
  sh[10] = 0.94617469575756001f * xy * (7.0f * z2 - 1.0f) * e4;
  sh[11] = 0.66904654355728916f * yz * (7.0f * z2 - 3.0f) * e4;
  sh[12] = 0.1057855469152043038f * (35.0f * z4 - 30.0f * z2 + 3.0f) * e4;
  sh[13] = 0.66904654355728916f * xz * (7.0f * z2 - 3.0f) * e4;
  sh[14] = 0.473087347878780009f * a * (7.0f * z2 - 1.0f) * e4;
  sh[15] = 1.77013076977993053f * xz * q * e4;
  sh[16] = 0.62583573544917613f * re4 * e4;
  sh[17] = 5.83141328139863895f * xy * (x2 * x4 - 7.0f * x4 * y2 + 7.0f * x2 * y4 - y2 * y4) * e8;
  sh[18] = 5.83141328139863895f * yz * im7 * e8;
  sh[19] = 1.06466553211908514f * xy * (15.0f * z2 - 1.0f) * (3.0f * x4 - 10.0f * x2 * y2 + 3.0f * y4) * e8;
  sh[20] = 3.44991062209810801f * yz * (5.0f * z2 - 1.0f) * im5 * e8;
  sh[21] = 1.91366609903732278f * xy * t4 * a * e8;
  sh[22] = 1.23526615529554407f * yz * t5 * p * e8;
  sh[23] = 0.91230451686981894f * xy * t6 * e8;
  sh[24] = 0.1090412458987799555f * yz * t7 * e8;
  sh[25] = 0.0090867704915649962938f *
           (6435.0f * z4 * z4 - 12012.0f * z4 * z2 + 6930.0f * z4 - 1260.0f * z2 + 35.0f) * e8;
  sh[26] = 0.1090412458987799555f * xz * t7 * e8;
  sh[27] = 0.456152258434909470f * t6 * a * e8;
  sh[28] = 1.23526615529554407f * xz * t5 * q * e8;
  sh[29] = 0.478416524759330697f * t4 * re4 * e8;
  sh[30] = 3.44991062209810801f * xz * (5.0f * z2 - 1.0f) * re5 * e8;
  sh[31] = 0.53233276605954257f * (15.0f * z2 - 1.0f) * (x2 * re5 - y2 * im5) * e8;
  sh[32] = 5.83141328139863895f * xz * re7 * e8;
  sh[33] = 0.72892666017482986f * (x2 * re7 - y2 * im7) * e8;
}

// ReLU as ONE instruction: v_max_i32 on the bits (as signed integers every negative float, and -0, is negative; positive floats
// keep their order) -- from fmaxf / fmed3 hipcc emits v_max(x, x) first (it canonicalises a possible sNaN), two VALU per value in
// every layer epilogue.  Deliberately NOT inline asm (rounds 1-3 had `asm("v_max_f32 %0, 0, %1")`): the compiler's hazard
// recogniser does not see an asm operand, and a ReLU placed right behind the MFMA that writes its input reads the register
// before the matrix pipe has written it (found in rsn_field_x6_train.hip, round 4).  -NaN -> 0, +NaN stays.
__device__ __forceinline__ float relu_f(float x) {
  const int xi = __float_as_int(x);
  return __int_as_float(xi > 0 ? xi : 0);
}
