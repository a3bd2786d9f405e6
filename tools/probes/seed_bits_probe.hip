// seed_bits_probe.hip -- the first GEMM of the analytic-normal sweep (rsn_field_kernel.h) in isolation: W_{L-1}^T times the
// density row masked by the ReLU bits of layer L-1, 256 x 256 over a 32-point tile, once as the fp32 loop the kernel had (32
// seed loads, masks and LDS writes, then gemm<8, 8, PF2> on v_mfma_f32_32x32x2_f32: 1,024 MFMAs of 64 cycles) and once as the
// bits form (gemm_bf16_bits, rsn_gemm_loops.h: the B operand built from the bits in registers, three pre-split bf16 pieces of
// V = W^T diag(w_density) per block and K = 16 step: 384 v_mfma_f32_32x32x16_bf16 of 32 cycles).  The bits form streams 384 KiB
// per wave and tile against 256 KiB, in a fifth of the MFMA cycles: does the 64 B/clk/CU L1 fill eat the gain?
// Four waves per workgroup, one workgroup per CU, every wave runs only this GEMM for TILES tiles; the four waves start together
// behind a barrier (all of them in the stream at once).  Two prefetch shapes: fragment buffers of half a K step (gemm_bf16's, 96
// registers) and a full K step ahead (192 registers: fits here, where the accumulators sit in AGPRs, but not beside the 128
// accumulator VGPRs of the product kernels, which are built with -amdgpu-mfma-vgpr-form).
// Cycles per tile come from a calibration launch of the same 1,024 fp32 MFMAs from registers (65,536 cycles by definition).
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I include -I reflect_sampling_nerf_amd/csrc \
//         tools/probes/seed_bits_probe.hip -o build/seed_bits_probe && build/seed_bits_probe
// Result: profiles/seed_bits_probe.txt.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rsn_epilogues.h"
#include "rsn_gemm_loops.h"
void rsn_set_error(const char*, ...) {}
#define CK(call) do { if ((call) != hipSuccess) { printf("%s failed\n", #call); exit(1); } } while (0)

#define TILES 64
#define SEG_F32 (32 * 8 * 256)       // floats of the fp32 segment [it 32][nb 8][lane][4]
#define SEG_B16 (16 * 8 * 3 * 256)   // floats of the three-piece segment [k16 16][nb 8][piece 3][lane][8 bf16]

// the bits form with a FULL K step of fragments in flight (two buffers of 8 x 3 fragments)
__device__ __forceinline__ void gemm_bits_full(f32x16 (&acc)[8], const float* __restrict__ wseg, const ReluBits<8>& m, int lane) {
  const WBuf wp = wbuf_make(wseg, lane);
  bf16x8 wa[8][3], wb[8][3];
  load_w16<8, 3>(wa, wp, 0, 8, 0);
  const SeedWords mw = seed_words<8>(m);
  bf16x8 bc = bits_bf16x8(mw, 0);
#pragma unroll 1
  for (int kk = 0; kk < 16; kk += 2) {
    load_w16<8, 3>(wb, wp, kk + 1, 8, 0);
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 bn = bits_bf16x8(mw, kk + 1);
    mma16_bits<8, 8>(acc, wa, bc, 0);
#pragma unroll
    for (int g = 0; g < 24; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int k2 = kk + 2 < 16 ? kk + 2 : 15;
    load_w16<8, 3>(wa, wp, k2, 8, 0);
    __builtin_amdgcn_sched_barrier(0);
    bc = bits_bf16x8(mw, k2);
    mma16_bits<8, 8>(acc, wb, bn, 0);
#pragma unroll
    for (int g = 0; g < 24; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// FORM 0: fp32 (seed loop + PF2 K loop, the training kernels' form); 1: bits, half-step buffers; 2: bits, a full step ahead;
// 3: calibration, 1,024 fp32 MFMAs from registers; 4: bits with the pieces formed in registers from the fp32 segment (gemm_f32_bits,
// the RSN_MMA_F32 kernel's form).  OWN: every wave streams its own copy of the segment (no L1 sharing).
template <int FORM, bool OWN>
__global__ __launch_bounds__(256) void k(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ wd,
                                          const unsigned* __restrict__ bits, float* out) {
  extern __shared__ float4 smem[];  // 32 KiB slab per wave, padded so that one workgroup fills the CU
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4* X = smem + wid * 32 * 64 + lane;
  const int h = lane >> 5;
  float s = 0.0f;
  __syncthreads();
  for (int t = 0; t < TILES; ++t) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const ReluBits<8> mb = load_relu_bits<8>(bits + (((size_t)blockIdx.x * 4 + wid) * TILES + t) * 256 + ln * 4);
    f32x16 acc[8];
    zero_acc<8>(acc);
    if (FORM == 0) {
#pragma unroll
      for (int it = 0; it < 32; ++it) {
        const float4 w = *reinterpret_cast<const float4*>(wd + it * 8 + 4 * h);
        const int word = mb.w[it / 8];
        const int base = ((it / 4) & 1) * 16 + 4 * (it & 3);
        X[it * 64] = make_float4(__uint_as_float(__float_as_uint(w.x) & bit_mask(word, base + 0)),
                                 __uint_as_float(__float_as_uint(w.y) & bit_mask(word, base + 1)),
                                 __uint_as_float(__float_as_uint(w.z) & bit_mask(word, base + 2)),
                                 __uint_as_float(__float_as_uint(w.w) & bit_mask(word, base + 3)));
      }
      gemm<8, 8, true>(acc, w32 + (OWN ? wid * SEG_F32 : 0), X, 32, ln);
    } else if (FORM == 1) {
      gemm_bf16_bits<8>(acc, w16 + (OWN ? wid * SEG_B16 : 0), mb, ln);
    } else if (FORM == 2) {
      gemm_bits_full(acc, w16 + (OWN ? wid * SEG_B16 : 0), mb, ln);
    } else if (FORM == 4) {
      gemm_f32_bits<8>(acc, w32 + (OWN ? wid * SEG_F32 : 0), wd, mb, ln);
    } else {
      const float4 w = make_float4(0.5f, 0.25f, -0.5f, 1.0f + 1e-3f * ln), b = make_float4(1.0f, 2.0f, 3.0f, (float)mb.w[0]);
#pragma unroll 1
      for (int it = 0; it < 32; ++it) {
        float4 wa[8];
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) wa[nb] = w;
        mma4<8>(acc, wa, b);
      }
    }
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) s += acc[nb][0] + acc[nb][5];
  }
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int FORM, bool OWN>
static double run(const char* name, const float* w32, const float* w16, const float* wd, const unsigned* bits, float* out, double cal_ms) {
  const int grid = 256;
  const size_t lds = 150 * 1024;
  CK(hipFuncSetAttribute((const void*)k<FORM, OWN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((k<FORM, OWN>), dim3(grid), dim3(256), lds, 0, w32, w16, wd, bits, out);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL((k<FORM, OWN>), dim3(grid), dim3(256), lds, 0, w32, w16, wd, bits, out);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.0f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  ms /= 5;
  if (hipGetLastError() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
  if (cal_ms > 0.0) printf("%-58s %8.3f ms  %8.0f cycles per tile\n", name, ms, ms / cal_ms * 65536.0);
  else printf("%-58s %8.3f ms  (= 65,536 cycles per tile)\n", name, ms);
  return ms;
}

int main() {
  float *w32, *w16, *wd, *out;
  unsigned* bits;
  const size_t nbits = 256ull * 4 * TILES * 256;
  CK(hipMalloc(&w32, 4ull * SEG_F32 * 4));
  CK(hipMalloc(&w16, 4ull * SEG_B16 * 4));
  CK(hipMalloc(&wd, 256 * 4));
  CK(hipMalloc(&out, 256 * 256 * 4));
  CK(hipMalloc(&bits, nbits * 4));
  std::vector<float> h(4ull * SEG_F32);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3f * (float)((i * 2654435761u) % 2001) - 1.0f;
  CK(hipMemcpy(w32, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  std::vector<unsigned short> hb(4ull * SEG_B16 * 2);  // bf16 bit patterns of small finite values
  for (size_t i = 0; i < hb.size(); ++i) hb[i] = (unsigned short)(0x3c00u + (i * 2654435761u) % 512u);
  CK(hipMemcpy(w16, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(wd, h.data(), 256 * 4, hipMemcpyHostToDevice));
  std::vector<unsigned> hm(nbits);
  for (size_t i = 0; i < nbits; ++i) hm[i] = (unsigned)(i * 2654435761u) ^ (unsigned)(i >> 3);
  CK(hipMemcpy(bits, hm.data(), nbits * 4, hipMemcpyHostToDevice));
  if (hipDeviceSynchronize() != hipSuccess) { printf("setup failed\n"); return 1; }
  printf("256 workgroups x 4 waves, %d tiles per wave, one 256 x 256 GEMM per tile\n", TILES);
  const double cal = run<3, false>("calibration: 1,024 fp32 MFMAs from registers", w32, w16, wd, bits, out, 0.0);
  printf("-- the four waves of a CU on the same segment\n");
  run<0, false>("fp32: seed loop + gemm<8, 8, PF2>", w32, w16, wd, bits, out, cal);
  run<1, false>("bits: half-step fragment buffers (gemm_bf16_bits)", w32, w16, wd, bits, out, cal);
  run<2, false>("bits: a full K step ahead", w32, w16, wd, bits, out, cal);
  run<4, false>("bits: pieces formed in registers (gemm_f32_bits)", w32, w16, wd, bits, out, cal);
  printf("-- every wave on its own copy of the segment (no L1 sharing between the waves)\n");
  run<0, true>("fp32: seed loop + gemm<8, 8, PF2>", w32, w16, wd, bits, out, cal);
  run<1, true>("bits: half-step fragment buffers (gemm_bf16_bits)", w32, w16, wd, bits, out, cal);
  run<2, true>("bits: a full K step ahead", w32, w16, wd, bits, out, cal);
  run<4, true>("bits: pieces formed in registers (gemm_f32_bits)", w32, w16, wd, bits, out, cal);
  return 0;
}
