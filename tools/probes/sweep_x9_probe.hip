// sweep_x9_probe.hip -- one W = 256 GEMM of the analytic-normal sweep (rsn_field_kernel.h, the loop over l behind the peeled seed
// GEMM) in isolation: W_l^T (256 x 256) times the masked layer gradient of a 32-point tile, the B operand read from the wave's LDS
// slab in the X layout.  Three forms:
//   (a) fp32: gemm<8, 8, PF2> over a wT_x segment, 1,024 v_mfma_f32_32x32x2_f32 of 64 cycles (what the kernel runs);
//   (b) nine products, packed: gemm_bf16<8, 3, FULL> over an hT_x segment (three bf16 pieces per weight, split on the host by
//       split_elem's expressions), 1,152 v_mfma_f32_32x32x16_bf16 of 32 cycles, 384 KiB of weights per wave and GEMM against 256;
//   (c) nine products, the weight pieces formed in registers from the fp32 segment (gemm_f32_x9, the RSN_MMA_F32 kernel's form:
//       the pieces of block b + 1 are formed under the nine MFMAs of block b);
// and, for scale, the six-product loop of the bf16x6 mode (gemm_bf16<8, 3>).
// The kernel's real grid: one workgroup of four waves per CU on every CU at once (clock and power effects show), each wave on its
// own 32-point tile and LDS slab, the workgroup's LDS sized so that one workgroup fills the CU; every wave runs only this GEMM for
// TILES tiles and the four waves start together behind a barrier.  Weights and activations are pseudo-random, not zeros: the
// clock the chip holds depends on the data.  What decides is the WALL time per tile (device events over five launches); cycles per
// tile come from a calibration launch of 1,024 fp32 MFMAs from registers (65,536 cycles by definition) and move with the clock.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I include -I reflect_sampling_nerf_amd/csrc \
//         tools/probes/sweep_x9_probe.hip -o build/sweep_x9_probe && build/sweep_x9_probe
// Result: profiles/sweep_x9_probe.txt.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rsn_mfma.h"
void rsn_set_error(const char*, ...) {}
#define CK(call) do { if ((call) != hipSuccess) { printf("%s failed\n", #call); exit(1); } } while (0)

#define TILES 64
#define SEG_F32 (32 * 8 * 256)       // floats of the fp32 segment [it 32][nb 8][lane][4]
#define SEG_B16 (16 * 8 * 3 * 256)   // floats of the three-piece segment [k16 16][nb 8][piece 3][lane][8 bf16]

// FORM 0: (a) fp32; 1: (b) nine products, packed pieces; 2: (c) nine products, pieces formed in registers; 3: calibration, 1,024
// fp32 MFMAs from registers; 4: six products (bf16x6).  OWN: every wave streams its own copy of the segment (no L1 sharing).
template <int FORM, bool OWN>
__global__ __launch_bounds__(256) void k(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ x0,
                                          float* out) {
  extern __shared__ float4 smem[];  // 32 KiB slab per wave, padded so that one workgroup fills the CU
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4* X = smem + wid * 32 * 64 + lane;
#pragma unroll 4
  for (int it = 0; it < 32; ++it) X[it * 64] = *reinterpret_cast<const float4*>(x0 + ((size_t)(wid * 32 + it) * 64 + lane) * 4);
  float s = 0.0f;
  __syncthreads();
  for (int t = 0; t < TILES; ++t) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    f32x16 acc[8];
    zero_acc<8>(acc);
    if (FORM == 0) {
      gemm<8, 8, true>(acc, w32 + (OWN ? wid * SEG_F32 : 0), X, 32, ln);
    } else if (FORM == 1) {
      gemm_bf16<8, 3, true>(acc, w16 + (OWN ? wid * SEG_B16 : 0), X, 16, ln);
    } else if (FORM == 2) {
      gemm_f32_x9<8>(acc, w32 + (OWN ? wid * SEG_F32 : 0), X, 16, ln);
    } else if (FORM == 4) {
      gemm_bf16<8, 3>(acc, w16 + (OWN ? wid * SEG_B16 : 0), X, 16, ln);
    } else {
      const float4 w = make_float4(0.5f, 0.25f, -0.5f, 1.0f + 1e-3f * ln), b = X[(t & 31) * 64];
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
    // the next tile's operand depends on this one's result (one slot, kept small: the values stay of order one)
    X[(t & 31) * 64].x = 0.5f + 1e-9f * s;
  }
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

static int g_grid = 256;

template <int FORM, bool OWN>
static double run(const char* name, const float* w32, const float* w16, const float* x0, float* out, double cal_ms, double ref_ms) {
  const size_t lds = 150 * 1024;
  CK(hipFuncSetAttribute((const void*)k<FORM, OWN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((k<FORM, OWN>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, out);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL((k<FORM, OWN>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, out);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.0f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  ms /= 5;
  if (hipGetLastError() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
  const double us_tile = ms * 1000.0 / TILES;
  if (cal_ms <= 0.0) printf("%-52s %8.3f ms  %7.2f us per tile  (= 65,536 cycles per tile)\n", name, ms, us_tile);
  else if (ref_ms <= 0.0) printf("%-52s %8.3f ms  %7.2f us per tile  %8.0f cycles per tile\n", name, ms, us_tile, ms / cal_ms * 65536.0);
  else printf("%-52s %8.3f ms  %7.2f us per tile  %8.0f cycles per tile  %.3f of (a)\n", name, ms, us_tile, ms / cal_ms * 65536.0, ms / ref_ms);
  return ms;
}

// round to nearest even, as the device's fp32 -> bf16 conversion (finite values)
static unsigned short bf16_rne(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
static float bf16_f32(unsigned short b) {
  const unsigned u = (unsigned)b << 16;
  float v;
  memcpy(&v, &u, 4);
  return v;
}

int main() {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  g_grid = prop.multiProcessorCount;
  float *w32, *w16, *x0, *out;
  CK(hipMalloc(&w32, 4ull * SEG_F32 * 4));
  CK(hipMalloc(&w16, 4ull * SEG_B16 * 4));
  CK(hipMalloc(&x0, 4ull * 32 * 64 * 4 * 4));
  CK(hipMalloc(&out, (size_t)g_grid * 256 * 4));
  std::vector<float> h(4ull * SEG_F32);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3f * (float)((i * 2654435761u) % 2001) - 1.0f;
  CK(hipMemcpy(w32, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  // the three pieces of the same weights in hT_x's layout (split_elem, rsn_pack.hip)
  std::vector<unsigned short> hb(4ull * SEG_B16 * 2);
  for (int c = 0; c < 4; ++c)
    for (int kk = 0; kk < 16; ++kk)
      for (int nb = 0; nb < 8; ++nb)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const float v = h[(size_t)c * SEG_F32 + ((size_t)((2 * kk + (e >> 2)) * 8 + nb) * 64 + lane) * 4 + (e & 3)];
            const unsigned short b1 = bf16_rne(v);
            const float r1 = v - bf16_f32(b1);
            const unsigned short b2 = bf16_rne(r1);
            const float r2 = r1 - bf16_f32(b2);
            const unsigned short b3 = bf16_rne(r2);
            const size_t base = (size_t)c * SEG_B16 * 2 + (size_t)(kk * 8 + nb) * 3 * 512 + (size_t)lane * 8 + e;
            hb[base] = b1; hb[base + 512] = b2; hb[base + 1024] = b3;
          }
  CK(hipMemcpy(w16, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  // activations: a masked gradient row -- about half the entries zero, the rest of order one
  std::vector<float> hx(4ull * 32 * 64 * 4);
  for (size_t i = 0; i < hx.size(); ++i) {
    const unsigned r = (unsigned)(i * 2246822519u) ^ (unsigned)(i >> 5);
    hx[i] = (r & 0x10000u) ? 0.0f : 1e-3f * (float)(r % 2001u) - 1.0f;
  }
  CK(hipMemcpy(x0, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  if (hipDeviceSynchronize() != hipSuccess) { printf("setup failed\n"); return 1; }
  printf("%d workgroups x 4 waves, %d tiles per wave, one 256 x 256 GEMM per 32-point tile, B from LDS\n", g_grid, TILES);
  const double cal = run<3, false>("calibration: 1,024 fp32 MFMAs from registers", w32, w16, x0, out, 0.0, 0.0);
  printf("-- the four waves of a CU on the same segment (the kernel's case)\n");
  const double a0 = run<0, false>("(a) fp32: gemm<8, 8, PF2>", w32, w16, x0, out, cal, 0.0);
  const double b0 = run<1, false>("(b) nine products, packed pieces (gemm_bf16 FULL)", w32, w16, x0, out, cal, a0);
  run<2, false>("(c) nine products, pieces in registers (gemm_f32_x9)", w32, w16, x0, out, cal, a0);
  run<4, false>("    six products (gemm_bf16<8, 3>)", w32, w16, x0, out, cal, a0);
  const double a1 = run<0, false>("(a) again", w32, w16, x0, out, cal, a0);
  const double b1 = run<1, false>("(b) again", w32, w16, x0, out, cal, a0);
  printf("-- every wave on its own copy of the segment (no L1 sharing between the waves)\n");
  const double a2 = run<0, true>("(a) fp32: gemm<8, 8, PF2>", w32, w16, x0, out, cal, 0.0);
  run<1, true>("(b) nine products, packed pieces (gemm_bf16 FULL)", w32, w16, x0, out, cal, a2);
  run<2, true>("(c) nine products, pieces in registers (gemm_f32_x9)", w32, w16, x0, out, cal, a2);
  run<4, true>("    six products (gemm_bf16<8, 3>)", w32, w16, x0, out, cal, a2);
  const double ratio = (b0 + b1) / (a0 + a1);
  printf("go / no-go: (b) / (a) wall time = %.3f (go at <= 0.850): %s\n", ratio, ratio <= 0.85 ? "GO" : "NO-GO");
  return 0;
}
