// sweep_x9_probe.hip -- one W = 256 GEMM of the analytic-normal sweep (rsn_field_kernel.h, the loop over l behind the peeled seed
// GEMM) in isolation: W_l^T (256 x 256) times the masked layer gradient of a 32-point tile, the B operand read from the wave's LDS
// slab in the X layout.  Five forms, (a) to (c) what the kernel ran in turn, (d) and (e) what it runs:
//   (a) fp32: gemm<8, 8, PF2> over a wT_x segment, 1,024 v_mfma_f32_32x32x2_f32 of 64 cycles;
//   (b) nine products, packed: gemm_bf16<8, 3, FULL> over an hT_x segment (three bf16 pieces per weight, split on the host by
//       split_elem's expressions), 1,152 v_mfma_f32_32x32x16_bf16 of 32 cycles, 384 KiB of weights per wave and GEMM against 256;
//   (c) nine products, the weight pieces formed in registers from the fp32 segment (gemm_f32_x9 below, the RSN_MMA_F32 kernel's
//       form until the sweep took shape (e): the pieces of block b + 1 are formed under the nine MFMAs of block b);
//   (d) nine products, packed, on v_mfma_f32_16x16x32_bf16: gemm_bf16_s16<8> over the same hT_x segment bytes (another per-lane
//       offset), 4,608 MFMAs of 16 cycles into the same 32-point x 256-row tile per wave: the same MFMA cycles, another shape;
//   (e) (d) with the weight pieces formed in registers from the fp32 segment (gemm_f32_s16, the RSN_MMA_F32 kernel's form);
// and, for scale, the six-product loop of the bf16x6 mode (gemm_bf16<8, 3>).
// The derivative GEMMs (the analytic-normal sweep, the backward sweep's dX) run (d) and (e) with SIX of the nine products, the three
// smallest left out (gemm_bf16_s16<8, 6>, gemm_f32_s16<8, 6>): forms (d6), (e6) and (d6) with the row stores in its K loop, checked on
// the integer operands like the others (every dropped product has a zero factor there) and timed against (d) and (d) with its stores:
// go per site at <= 0.85 of the nine-product form's time.
// The backward sweep runs the same GEMMs and keeps, per GEMM, the 32 KiB of layer-gradient rows it reads in a row-major
// [points, 256] buffer.  Three more forms for it: (a) with the stores in its K loop (gemm_run2's saver, what that sweep ran), (d)
// with them in its K loop (gemm_bf16_s16's saver, checked first on the integer operands: result, rows and rows past the valid
// ones), and (d) with the result rows stored from the epilogue; the go / no-go is the better placement against (a) with its stores.
// The training forward's trunk runs W_l (256 x 256) the same way behind a bias start and in front of a ReLU epilogue: three more forms
// (kf / fwd_tile below: the fp32 loop with store_act_init, the packed and the in-register 16-shape with store_act16_relu_init),
// checked first on integer operands (slab, mask words, restarted accumulators, kept rows, stray stores), then timed tile feeding tile.
// Before anything is timed, (b) and (d) run one tile each on integer operands whose every sum is exact in fp32 (19-bit weights
// against 0 / +-1 activations, then the reverse) and their X slabs are compared with each other and with the host's integer sums.
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

#include "rsn_epilogues.h"
#include "rsn_gemm_loops.h"
void rsn_set_error(const char*, ...) {}
#define CK(call) do { if ((call) != hipSuccess) { printf("%s failed\n", #call); exit(1); } } while (0)

// The 32x32x16 form of the in-register loop, as the RSN_MMA_F32 kernel ran it before the sweep moved to the 16x16x32 shape; kept
// here as form (c), what form (e) is measured against.  gemm_bf16<NBO, 3, true> with the weight pieces formed by split8<3> from the
// fp32 fragments of a wT_* segment ([it][NBO][lane][4]; K-iterations 2kk, 2kk + 1 are the eight values of K = 16 step kk), the nine
// products in mma16<.., true>'s order.  K a multiple of 16.
// the nine products of one block and K step, in mma16<.., true>'s order
__device__ __forceinline__ f32x16 x9_block(f32x16 c, const BSplit& w, const BSplit& b) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s3, b.s3, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s3, b.s2, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s2, b.s3, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s3, b.s1, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s2, b.s2, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s1, b.s3, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s2, b.s1, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s1, b.s2, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.s1, b.s1, c, 0, 0, 0);
  return c;
}

// A software pipeline over the blocks: while the nine MFMAs of block b run (288 cycles), the VALU forms the pieces of block b + 1
// (about 50 instructions, five or six behind each MFMA; the last block of a K step also splits the next step's activations).  A
// fragment buffer is dead once its last block is split, and is reloaded for the next K step at the start of the block after that.
// Written block by block (split, then nine MFMAs) hipcc issues the ~50 VALU instructions of a block in one run ahead of its MFMAs:
// that loop took 0.98 of the fp32 form's time alone and made the unfolded training forward 7 % slower; this one 0.87-0.90
// (tools/probes/sweep_x9_probe.hip), the forward 2 % faster.
template <int NBO>
__device__ __forceinline__ void gemm_f32_x9(f32x16 (&acc)[NBO], const float* __restrict__ w32seg, const float4* xl, int n_k16,
                                            int lane) {
  static_assert(NBO % 2 == 0, "two fragment buffers of NBO / 2 blocks");
  constexpr int NH = NBO / 2;
  const WBuf wp = wbuf_make(w32seg, lane);
  float4 fa[NH][2], fb[NH][2];
  load_w32_pair<NBO, NH>(fa, wp, 0, 0);
  load_w32_pair<NBO, NH>(fb, wp, 0, NH);
  BSplit bc = split8<3>(xl[0], xl[64]);
  const int k1 = n_k16 > 1 ? 1 : 0;
  float4 xlo = xl[(2 * k1) * 64], xhi = xl[(2 * k1 + 1) * 64];  // fp32 activations of the NEXT K step
  BSplit w = split8<3>(fa[0][0], fa[0][1]);
  BSplit bn = bc;
#pragma unroll 1
  for (int kk = 0; kk < n_k16; ++kk) {
    const int kn = (kk + 1 < n_k16) ? kk + 1 : kk;  // clamped: one control path keeps the s_waitcnt counts exact
    const int k2 = (kk + 2 < n_k16) ? kk + 2 : kn;
#pragma unroll
    for (int b = 0; b < NBO; ++b) {
      BSplit wn;
      if (b + 1 < NH) wn = split8<3>(fa[b + 1][0], fa[b + 1][1]);
      else if (b + 1 < NBO) wn = split8<3>(fb[b + 1 - NH][0], fb[b + 1 - NH][1]);
      else wn = split8<3>(fa[0][0], fa[0][1]);  // block 0 of step kn: fa was reloaded at block NH - 1
      if (b == NH - 1) load_w32_pair<NBO, NH>(fa, wp, kn, 0);
      if (b == NBO - 1) {
        load_w32_pair<NBO, NH>(fb, wp, kn, NH);
        bn = split8<3>(xlo, xhi);
        xlo = xl[(2 * k2) * 64];
        xhi = xl[(2 * k2 + 1) * 64];
      }
      acc[b] = x9_block(acc[b], w, bc);
      const bool loads = b == NH - 1 || b == NBO - 1;
#pragma unroll
      for (int g = 0; g < 9; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        if (loads && g < 2 * NH) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
        if (b == NBO - 1) __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);  // the next block's pieces + the next step's activations
        else __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);  // the next block's pieces
      }
      if (b == NBO - 1) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // the LDS reads of the activations
      __builtin_amdgcn_sched_barrier(0);
      w = wn;
    }
    bc = bn;
  }
}

#define TILES 64
#define SEG_F32 (32 * 8 * 256)       // floats of the fp32 segment [it 32][nb 8][lane][4]
#define SEG_B16 (16 * 8 * 3 * 256)   // floats of the three-piece segment [k16 16][nb 8][piece 3][lane][8 bf16]
#define ROW_SLOTS 16                 // saved-row tiles per wave, walked round: 1,024 waves x 16 x 32 KiB = 512 MiB, beyond every cache

// The backward sweep's GEMMs keep the rows they read (forms 7 to 9): the epilogue variant of the 16-shape, every result float4 to
// its row (the float4 store_masked_bits16 writes to the slab: K-iteration 4 nb + 2 rh + kh of old lane ol + 16 ph) -- a burst of 32
// stores behind the K loop.  `b`: rowbuf(.., m = L & 15, h = (L >> 4) & 1).
template <int NBO>
__device__ __forceinline__ void store_rows16(const f32x4 (&acc)[NBO][2][2], const RowBuf& b, int lane) {
  const unsigned at = b.voff + (unsigned)(lane >> 5) * 32u;
#pragma unroll
  for (int ph = 0; ph < 2; ++ph)
#pragma unroll
    for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
      for (int rh = 0; rh < 2; ++rh) {
        const f32x4& a = acc[nb][rh][ph];
        const u32x4 o = {__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])};
        __builtin_amdgcn_raw_buffer_store_b128(o, b.r, at + (unsigned)ph * 16u * b.lim + (unsigned)((nb * 4 + 2 * rh) * 32), 0,
                                               RSN_SAVED_ROW_AUX);
      }
}

// FORM 0: (a) fp32; 1: (b) nine products, packed pieces; 2: (c) nine products, pieces formed in registers; 3: calibration, 1,024
// fp32 MFMAs from registers; 4: six products (bf16x6); 5: (d) nine products, packed pieces, 16x16x32; 6: (e) the same, pieces formed in registers;
// 7: (d) keeping the rows it reads, stores in the K loop (gemm_bf16_s16's saver); 8: (a) keeping them, stores in the K loop (gemm_run2's
// saver: what the backward sweep ran); 9: (d) with the result rows stored from the epilogue (store_rows16);
// 10: (d) with six products (the analytic-normal sweep's form); 11: 10 keeping the rows it reads, stores in the K loop (the backward
// sweep's form); 12: (e) with six products.
// OWN: every wave streams its own copy of the segment (no L1 sharing).
template <int FORM, bool OWN>
__global__ __launch_bounds__(256) void k(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ x0,
                                          float* out, float* rowsbuf = nullptr) {
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
    // this tile's 32 rows of the row-major [points, 256] buffer (wave-uniform base)
    const long long row0 = ((long long)(blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wid)) * ROW_SLOTS + (t % ROW_SLOTS)) * 32 * 256;
    if constexpr (FORM == 5 || FORM == 6 || FORM == 7 || FORM == 9 || FORM == 10 || FORM == 11 || FORM == 12) {
      f32x4 a16[8][2][2];
      zero_acc16<8>(a16);
      if (FORM == 5) gemm_bf16_s16<8, 9>(a16, w16 + (OWN ? wid * SEG_B16 : 0), X, 8, ln);
      else if (FORM == 7) gemm_bf16_s16<8, 9>(a16, w16 + (OWN ? wid * SEG_B16 : 0), X, 8, ln, rowbuf<false>(rowsbuf, row0, 32, 256, ln & 15, (ln >> 4) & 1));
      else if (FORM == 9) {
        gemm_bf16_s16<8, 9>(a16, w16 + (OWN ? wid * SEG_B16 : 0), X, 8, ln);
        store_rows16<8>(a16, rowbuf<false>(rowsbuf, row0, 32, 256, ln & 15, (ln >> 4) & 1), ln);
      }
      else if (FORM == 10) gemm_bf16_s16<8, 6>(a16, w16 + (OWN ? wid * SEG_B16 : 0), X, 8, ln);
      else if (FORM == 11) gemm_bf16_s16<8, 6>(a16, w16 + (OWN ? wid * SEG_B16 : 0), X, 8, ln, rowbuf<false>(rowsbuf, row0, 32, 256, ln & 15, (ln >> 4) & 1));
      else if (FORM == 12) gemm_f32_s16<8, 6>(a16, w32 + (OWN ? wid * SEG_F32 : 0), X, 8, ln);
      else gemm_f32_s16<8, 9>(a16, w32 + (OWN ? wid * SEG_F32 : 0), X, 8, ln);
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) s += (a16[nb][0][0][0] + a16[nb][0][1][1]) + (a16[nb][1][0][2] + a16[nb][1][1][3]);
      X[(t & 31) * 64].x = 0.5f + 1e-9f * s;
      continue;
    }
    f32x16 acc[8];
    zero_acc<8>(acc);
    if (FORM == 0) {
      gemm<8, 8, true>(acc, w32 + (OWN ? wid * SEG_F32 : 0), X, 32, ln);
    } else if (FORM == 8) {
      gemm<8, 8, true>(acc, w32 + (OWN ? wid * SEG_F32 : 0), X, 32, ln, rowbuf<false>(rowsbuf, row0, 32, 256, ln & 31, ln >> 5));
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

// The training forward's trunk runs the same W x W GEMM per layer with the ReLU epilogue behind it: the accumulators start from the
// layer's bias, the GEMM keeps the rows it reads (act[l-1], 32 KiB per tile, stores in its K loop), and the epilogue writes the
// relu'd result to the slab -- the next GEMM's operand -- with the layer's mask words (1 KiB per tile) and restarts the
// accumulators from the next bias.  Three forms, every tile feeding the next as the layers do (weights scaled so that the
// activations stay of order one):
//   FORM 0: the fp32 loop as the kernel ran it (gemm_run2 with its saver, first fragment fetched ahead of store_act_init);
//   FORM 1: gemm_bf16_s16 with its saver + store_act16_relu_init (the RSN_MMA_F32_FOLDED kernel's form);
//   FORM 2: gemm_f32_s16 with its saver + store_act16_relu_init (the RSN_MMA_F32 kernel's form).
template <int FORM>
__device__ __forceinline__ void fwd_tile(f32x16 (&acc)[8], f32x4 (&a16)[8][2][2], float4 (&wa)[8], const float* __restrict__ w32,
                                         const float* __restrict__ w16, float4* X, const float* __restrict__ bias, float* rows,
                                         long long row0, int valid, unsigned* bits32, int ln) {
  if constexpr (FORM == 0) {
    gemm_run2<8, 8>(acc, wa, w32, X, 32, ln, rowbuf<false>(rows, row0, valid, 256, ln & 31, ln >> 5));
    pre_w<8>(wa, w32, ln);
    const int m = ln & 31, h = ln >> 5;
    store_act_init<8, true, false>(acc, X, (float*)nullptr, h, bias, m < valid ? bits32 + (m * 2 + h) * 4 : nullptr);
  } else {
    const RowBuf rb = rowbuf<false>(rows, row0, valid, 256, ln & 15, (ln >> 4) & 1);
    if constexpr (FORM == 1) gemm_bf16_s16<8, 9>(a16, w16, X, 8, ln, rb); else gemm_f32_s16<8, 9>(a16, w32, X, 8, ln, rb);
    const int m = (ln & 15) + 16 * (ln >> 5), h = (ln >> 4) & 1;
    store_act16_relu_init<8>(a16, X, ln, bias, m < valid ? bits32 + (m * 2 + h) * 4 : nullptr);
  }
}

template <int FORM>
__global__ __launch_bounds__(256) void kf(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ x0,
                                           const float* __restrict__ bias, float* out, float* rowsbuf, unsigned* bitsbuf) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4* X = smem + wid * 32 * 64 + lane;
#pragma unroll 4
  for (int it = 0; it < 32; ++it) X[it * 64] = *reinterpret_cast<const float4*>(x0 + ((size_t)(wid * 32 + it) * 64 + lane) * 4);
  f32x16 acc[8];
  f32x4 a16[8][2][2];
  float4 wa[8];
  if constexpr (FORM == 0) { init_acc<8>(acc, bias, lane >> 5); pre_w<8>(wa, w32, lane); } else init_acc16<8>(a16, bias, lane);
  __syncthreads();
  for (int t = 0; t < TILES; ++t) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const long long slot = (long long)(blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wid)) * ROW_SLOTS + (t % ROW_SLOTS);
    fwd_tile<FORM>(acc, a16, wa, w32, w16, X, bias, rowsbuf, slot * 32 * 256, 32, bitsbuf + slot * 32 * 8, ln);
  }
  out[blockIdx.x * 256 + threadIdx.x] = X[0].x + X[17 * 64].y;
}

// one wave, one tile of a forward form on integer operands: the slab behind the epilogue, the mask words, the rows the GEMM kept
// (`valid` of 32 inside the descriptor) and, through a second plain epilogue, the accumulators as the epilogue restarted them
template <int FORM>
__global__ __launch_bounds__(64) void chkf(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ x0,
                                            const float* __restrict__ bias, float* out, float* out2, float* rows, unsigned* bits, int valid) {
  __shared__ float4 slab[32 * 64];
  const int lane = threadIdx.x;
  float4* X = slab + lane;
  for (int it = 0; it < 32; ++it) X[it * 64] = *reinterpret_cast<const float4*>(x0 + ((size_t)it * 64 + lane) * 4);
  __syncthreads();
  f32x16 acc[8];
  f32x4 a16[8][2][2];
  float4 wa[8];
  if constexpr (FORM == 0) { init_acc<8>(acc, bias, lane >> 5); pre_w<8>(wa, w32, lane); } else init_acc16<8>(a16, bias, lane);
  fwd_tile<FORM>(acc, a16, wa, w32, w16, X, bias + 256, rows, 0, valid, bits, lane);
  __syncthreads();
  for (int it = 0; it < 32; ++it) *reinterpret_cast<float4*>(out + ((size_t)it * 64 + lane) * 4) = X[it * 64];
  __syncthreads();
  if constexpr (FORM == 0) store_act<8, 8, false>(acc, X); else store_act16<8>(a16, X, lane);
  __syncthreads();
  for (int it = 0; it < 32; ++it) *reinterpret_cast<float4*>(out2 + ((size_t)it * 64 + lane) * 4) = X[it * 64];
}

// one wave, one tile: the GEMM of form (b), (d), (e), (d6) = 10 or (e6) = 12, its result written to the X slab by the form's own epilogue and copied out
template <int FORM>
__global__ __launch_bounds__(64) void chk(const float* __restrict__ w32, const float* __restrict__ w16, const float* __restrict__ x0, float* out) {
  __shared__ float4 slab[32 * 64];
  const int lane = threadIdx.x;
  float4* X = slab + lane;
  for (int it = 0; it < 32; ++it) X[it * 64] = *reinterpret_cast<const float4*>(x0 + ((size_t)it * 64 + lane) * 4);
  __syncthreads();
  if constexpr (FORM == 5 || FORM == 6 || FORM == 10 || FORM == 12) {
    f32x4 a16[8][2][2];
    zero_acc16<8>(a16);
    if (FORM == 5) gemm_bf16_s16<8, 9>(a16, w16, X, 8, lane);
    else if (FORM == 10) gemm_bf16_s16<8, 6>(a16, w16, X, 8, lane);
    else if (FORM == 12) gemm_f32_s16<8, 6>(a16, w32, X, 8, lane);
    else gemm_f32_s16<8, 9>(a16, w32, X, 8, lane);
    __syncthreads();
    store_act16<8>(a16, X, lane);
  } else {
    f32x16 acc[8];
    zero_acc<8>(acc);
    gemm_bf16<8, 3, true>(acc, w16, X, 16, lane);
    __syncthreads();
    store_act<8, 8, false>(acc, X);
  }
  __syncthreads();
  for (int it = 0; it < 32; ++it) *reinterpret_cast<float4*>(out + ((size_t)it * 64 + lane) * 4) = X[it * 64];
}

// one wave, one tile: form (d) (NP = 9) or (d6) (NP = 6) keeping the rows it reads (gemm_bf16_s16's saver) with `valid` of the 32
// rows inside the descriptor
template <int NP>
__global__ __launch_bounds__(64) void chk_rows(const float* __restrict__ w16, const float* __restrict__ x0, float* out, float* rows, int valid) {
  __shared__ float4 slab[32 * 64];
  const int lane = threadIdx.x;
  float4* X = slab + lane;
  for (int it = 0; it < 32; ++it) X[it * 64] = *reinterpret_cast<const float4*>(x0 + ((size_t)it * 64 + lane) * 4);
  __syncthreads();
  f32x4 a16[8][2][2];
  zero_acc16<8>(a16);
  gemm_bf16_s16<8, NP>(a16, w16, X, 8, lane, rowbuf<false>(rows, 0, valid, 256, lane & 15, (lane >> 4) & 1));
  __syncthreads();
  store_act16<8>(a16, X, lane);
  __syncthreads();
  for (int it = 0; it < 32; ++it) *reinterpret_cast<float4*>(out + ((size_t)it * 64 + lane) * 4) = X[it * 64];
}

static int g_grid = 256;
static float* g_rows = nullptr;  // [g_grid x 4 waves x ROW_SLOTS x 32 points, 256] saved rows of forms 7 to 9

template <int FORM, bool OWN>
static double run(const char* name, const float* w32, const float* w16, const float* x0, float* out, double cal_ms, double ref_ms) {
  const size_t lds = 150 * 1024;
  CK(hipFuncSetAttribute((const void*)k<FORM, OWN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((k<FORM, OWN>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, out, g_rows);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL((k<FORM, OWN>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, out, g_rows);
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

// one fp32 segment [it 32][nb 8][lane][4] as its three bf16 pieces [k16 16][nb 8][piece 3][lane][8] (split_elem, rsn_pack.hip)
static void pack_pieces(const float* h, unsigned short* hb) {
  for (int kk = 0; kk < 16; ++kk)
    for (int nb = 0; nb < 8; ++nb)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const float v = h[((size_t)((2 * kk + (e >> 2)) * 8 + nb) * 64 + lane) * 4 + (e & 3)];
          const unsigned short b1 = bf16_rne(v);
          const float r1 = v - bf16_f32(b1);
          const unsigned short b2 = bf16_rne(r1);
          const float r2 = r1 - bf16_f32(b2);
          const unsigned short b3 = bf16_rne(r2);
          const size_t base = (size_t)(kk * 8 + nb) * 3 * 512 + (size_t)lane * 8 + e;
          hb[base] = b1; hb[base + 512] = b2; hb[base + 1024] = b3;
        }
}

// Forms (b), (d), (e) and their six-product forms on integer operands: `wide` weights of up to 19 bits against activations in
// {0, +-1}, fifteen in sixteen zero, or the reverse.  (With nearest-rounding pieces an integer below 2^17 has no lo piece; from 2^18
// on hi, mid and lo are all there, so every kept product of the six-product forms -- w_lo b_hi, w_mid b_hi, w_hi b_lo, w_hi b_mid
// among them -- carries part of the sums.  w_mid b_mid needs both operands wide: tests/test_six_products_gpu.py has random operands
// for that.)  The sum of the magnitudes of every dot product stays under 2^24 / 1.01^2 (checked below), so any order of accumulation
// of any pieces gives the integer result.
static bool check_forms(bool wide_w, float* w32, float* w16, float* x0, float* out) {
  std::vector<float> hw(SEG_F32), hx(32 * 64 * 4);
  auto big = [](size_t i) { return (float)((long long)((i * 2654435761u + 12345u) % 1048575u) - 524287); };
  auto small = [](size_t i) { const unsigned r = (unsigned)(i * 2246822519u) >> 13; return (r & 60u) ? 0.0f : ((r & 1u) ? 1.0f : -1.0f); };
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = wide_w ? big(i) : small(i);
  for (size_t i = 0; i < hx.size(); ++i) hx[i] = wide_w ? small(i + 7) : big(i + 7);
  std::vector<unsigned short> hb((size_t)SEG_B16 * 2);
  pack_pieces(hw.data(), hb.data());
  CK(hipMemcpy(w32, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(w16, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(x0, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> ob(hx.size()), od(hx.size()), oe(hx.size());
  hipLaunchKernelGGL((chk<1>), dim3(1), dim3(64), 0, 0, w32, w16, x0, out);
  CK(hipMemcpy(ob.data(), out, ob.size() * 4, hipMemcpyDeviceToHost));
  hipLaunchKernelGGL((chk<5>), dim3(1), dim3(64), 0, 0, w32, w16, x0, out);
  CK(hipMemcpy(od.data(), out, od.size() * 4, hipMemcpyDeviceToHost));
  hipLaunchKernelGGL((chk<6>), dim3(1), dim3(64), 0, 0, w32, w16, x0, out);
  CK(hipMemcpy(oe.data(), out, oe.size() * 4, hipMemcpyDeviceToHost));
  std::vector<float> od6(hx.size()), oe6(hx.size());
  hipLaunchKernelGGL((chk<10>), dim3(1), dim3(64), 0, 0, w32, w16, x0, out);
  CK(hipMemcpy(od6.data(), out, od6.size() * 4, hipMemcpyDeviceToHost));
  hipLaunchKernelGGL((chk<12>), dim3(1), dim3(64), 0, 0, w32, w16, x0, out);
  CK(hipMemcpy(oe6.data(), out, oe6.size() * 4, hipMemcpyDeviceToHost));
  size_t bad_b = 0, bad_d = 0, bad_e = 0, differ = 0, bad_d6 = 0, bad_e6 = 0;
  double worst_abs = 0.0;  // largest sum of |w| |x| over a dot product
  for (int it = 0; it < 32; ++it)      // X[it][lane][c]: row 8 it + 4 (lane >> 5) + c of point lane & 31
    for (int lane = 0; lane < 64; ++lane)
      for (int c = 0; c < 4; ++c) {
        const int row = 8 * it + 4 * (lane >> 5) + c, p = lane & 31;
        long long ref = 0, mag = 0;
        for (int ki = 0; ki < 32; ++ki)
          for (int kh = 0; kh < 2; ++kh)
            for (int kc = 0; kc < 4; ++kc) {
              const long long t = (long long)hw[((size_t)(ki * 8 + row / 32) * 64 + (row % 32) + 32 * kh) * 4 + kc] *
                                  (long long)hx[((size_t)ki * 64 + p + 32 * kh) * 4 + kc];
              ref += t;
              mag += t < 0 ? -t : t;
            }
        if ((double)mag > worst_abs) worst_abs = (double)mag;
        const size_t o = ((size_t)it * 64 + lane) * 4 + c;
        bad_b += ob[o] != (float)ref;
        bad_d += od[o] != (float)ref;
        bad_e += oe[o] != (float)ref;
        bad_d6 += od6[o] != (float)ref;
        bad_e6 += oe6[o] != (float)ref;
        differ += ob[o] != od[o] || od[o] != oe[o];
      }
  printf("check, %s: (b) wrong %zu, (d) wrong %zu, (e) wrong %zu, not all equal %zu of %zu\n",
         wide_w ? "19-bit weights x 0/+-1 activations" : "0/+-1 weights x 19-bit activations", bad_b, bad_d, bad_e, differ, ob.size());
  printf("check, %s: six products: (d6) wrong %zu, (e6) wrong %zu of %zu; largest sum of magnitudes %.0f (%.3f of 2^24)\n",
         wide_w ? "19-bit weights x 0/+-1 activations" : "0/+-1 weights x 19-bit activations", bad_d6, bad_e6, ob.size(), worst_abs,
         worst_abs / 16777216.0);
  if (worst_abs * 1.0201 >= 16777216.0) { printf("the integer case is not exact in every order\n"); return false; }
  // (d) with the row saver: the same result, every float4 it read in its row of a [points, 256] buffer (row m, floats 8 it + 4 h
  // .. of slab entry (it, old lane m + 32 h)), rows at or past `valid` and the guard rows behind the tile untouched
  size_t bad_r = 0, bad_s = 0, stray = 0;
  const int guard = 8;
  std::vector<unsigned> hr((size_t)(32 + guard) * 256);
  for (int pass = 0; pass < 6; ++pass) {  // (d), then (d6): the same result, rows and silence past the valid rows
    const int valid = pass % 3 == 0 ? 32 : (pass % 3 == 1 ? 19 : 1);
    CK(hipMemset(g_rows, 0xCD, hr.size() * 4));
    if (pass < 3) hipLaunchKernelGGL(chk_rows<9>, dim3(1), dim3(64), 0, 0, w16, x0, out, g_rows, valid);
    else hipLaunchKernelGGL(chk_rows<6>, dim3(1), dim3(64), 0, 0, w16, x0, out, g_rows, valid);
    CK(hipMemcpy(oe.data(), out, oe.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hr.data(), g_rows, hr.size() * 4, hipMemcpyDeviceToHost));
    for (size_t o = 0; o < od.size(); ++o) bad_r += oe[o] != od[o];
    for (int m = 0; m < 32 + guard; ++m)
      for (int f = 0; f < 256; ++f) {
        const unsigned got = hr[(size_t)m * 256 + f];
        if (m >= valid) { stray += got != 0xCDCDCDCDu; continue; }
        const float want = hx[((size_t)(f / 8) * 64 + m + 32 * ((f / 4) & 1)) * 4 + (f & 3)];
        unsigned wb;
        memcpy(&wb, &want, 4);
        bad_s += got != wb;
      }
  }
  printf("check, %s: (d) and (d6) with the row saver, 32 / 19 / 1 valid rows: result differs from (d) %zu, saved rows wrong %zu, stray stores %zu\n",
         wide_w ? "19-bit weights x 0/+-1 activations" : "0/+-1 weights x 19-bit activations", bad_r, bad_s, stray);
  return bad_b == 0 && bad_d == 0 && bad_e == 0 && differ == 0 && bad_d6 == 0 && bad_e6 == 0 && bad_r == 0 && bad_s == 0 && stray == 0;
}

static float* g_bias = nullptr;     // two biases of 256 (the layer's, the next layer's)
static unsigned* g_bits = nullptr;  // mask words, 256 per tile, laid out like the saved rows

// The three forward forms on the integer operands of check_forms(true) with integer biases: the relu'd slab, the mask words in
// ReluBits' layout ([point][half][4 words]: unit 32 nb + 8 q + 4 h + j is bit 16 (nb & 1) + 4 q + j of word nb / 2), the restarted
// accumulators, the kept rows, and nothing written for rows at or past `valid`.
static bool check_fwd(float* w32, float* w16, float* x0, float* out) {
  std::vector<float> hw(SEG_F32), hx(32 * 64 * 4), hbias(512);
  auto big = [](size_t i) { return (float)((long long)((i * 2654435761u + 12345u) % 262143u) - 131071); };
  auto small = [](size_t i) { const unsigned r = (unsigned)(i * 2246822519u) >> 13; return (r & 12u) ? 0.0f : ((r & 1u) ? 1.0f : -1.0f); };
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = big(i);
  for (size_t i = 0; i < hx.size(); ++i) hx[i] = small(i + 7);
  for (int r = 0; r < 256; ++r) { hbias[r] = (float)((r * 37) % 201 - 100); hbias[256 + r] = (float)((r * 11) % 61 - 30); }
  std::vector<unsigned short> hb((size_t)SEG_B16 * 2);
  pack_pieces(hw.data(), hb.data());
  CK(hipMemcpy(w32, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(w16, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(x0, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(g_bias, hbias.data(), hbias.size() * 4, hipMemcpyHostToDevice));
  std::vector<long long> ref(256 * 32);
  for (int row = 0; row < 256; ++row)
    for (int p = 0; p < 32; ++p) {
      long long s = (long long)hbias[row];
      for (int ki = 0; ki < 32; ++ki)
        for (int kh = 0; kh < 2; ++kh)
          for (int kc = 0; kc < 4; ++kc)
            s += (long long)hw[((size_t)(ki * 8 + row / 32) * 64 + (row % 32) + 32 * kh) * 4 + kc] * (long long)hx[((size_t)ki * 64 + p + 32 * kh) * 4 + kc];
      ref[row * 32 + p] = s;
    }
  const int guard = 8;
  std::vector<float> o1(hx.size()), o2(hx.size());
  std::vector<unsigned> hr((size_t)(32 + guard) * 256), hm((size_t)(32 + guard) * 8);
  bool ok = true;
  for (int form = 0; form < 3; ++form) {
    size_t bad_x = 0, bad_a = 0, bad_s = 0, bad_m = 0, stray = 0;
    for (int valid : {32, 19, 1}) {
      CK(hipMemset(g_rows, 0xCD, hr.size() * 4));
      CK(hipMemset(g_bits, 0xCD, hm.size() * 4));
      if (form == 0) hipLaunchKernelGGL((chkf<0>), dim3(1), dim3(64), 0, 0, w32, w16, x0, g_bias, out, out + 8192, g_rows, g_bits, valid);
      else if (form == 1) hipLaunchKernelGGL((chkf<1>), dim3(1), dim3(64), 0, 0, w32, w16, x0, g_bias, out, out + 8192, g_rows, g_bits, valid);
      else hipLaunchKernelGGL((chkf<2>), dim3(1), dim3(64), 0, 0, w32, w16, x0, g_bias, out, out + 8192, g_rows, g_bits, valid);
      CK(hipMemcpy(o1.data(), out, o1.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(o2.data(), out + 8192, o2.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hr.data(), g_rows, hr.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hm.data(), g_bits, hm.size() * 4, hipMemcpyDeviceToHost));
      for (int it = 0; it < 32; ++it)
        for (int lane = 0; lane < 64; ++lane)
          for (int c = 0; c < 4; ++c) {
            const int row = 8 * it + 4 * (lane >> 5) + c, p = lane & 31;
            const long long z = ref[row * 32 + p];
            const size_t o = ((size_t)it * 64 + lane) * 4 + c;
            bad_x += o1[o] != (float)(z > 0 ? z : 0);
            bad_a += o2[o] != hbias[256 + row];
            if (p < valid) {
              const int nb = row / 32, q = (row % 32) / 8, h = (row % 8) / 4, j = row % 4;
              bad_m += ((hm[(size_t)(p * 2 + h) * 4 + nb / 2] >> (16 * (nb & 1) + 4 * q + j)) & 1u) != (unsigned)(z > 0);
            }
          }
      for (int m = 0; m < 32 + guard; ++m) {
        for (int w = 0; w < 8; ++w) stray += m >= valid && hm[(size_t)m * 8 + w] != 0xCDCDCDCDu;
        for (int f = 0; f < 256; ++f) {
          const unsigned got = hr[(size_t)m * 256 + f];
          if (m >= valid) { stray += got != 0xCDCDCDCDu; continue; }
          const float want = hx[((size_t)(f / 8) * 64 + m + 32 * ((f / 4) & 1)) * 4 + (f & 3)];
          unsigned wb;
          memcpy(&wb, &want, 4);
          bad_s += got != wb;
        }
      }
    }
    printf("check, forward form %d (0 fp32 loop, 1 packed 16-shape, 2 in-register 16-shape), 32 / 19 / 1 valid rows: slab wrong %zu, "
           "restarted accumulators wrong %zu, mask bits wrong %zu, kept rows wrong %zu, stray stores %zu\n", form, bad_x, bad_a, bad_m, bad_s, stray);
    ok = ok && bad_x == 0 && bad_a == 0 && bad_m == 0 && bad_s == 0 && stray == 0;
  }
  return ok;
}

template <int FORM>
static double run_fwd(const char* name, const float* w32, const float* w16, const float* x0, float* out, double cal_ms, double ref_ms) {
  const size_t lds = 150 * 1024;
  CK(hipFuncSetAttribute((const void*)kf<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((kf<FORM>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, g_bias, out, g_rows, g_bits);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL((kf<FORM>), dim3(g_grid), dim3(256), lds, 0, w32, w16, x0, g_bias, out, g_rows, g_bits);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.0f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  ms /= 5;
  if (hipGetLastError() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
  if (ref_ms <= 0.0) printf("%-52s %8.3f ms  %7.2f us per tile  %8.0f cycles per tile\n", name, ms, ms * 1000.0 / TILES, ms / cal_ms * 65536.0);
  else printf("%-52s %8.3f ms  %7.2f us per tile  %8.0f cycles per tile  %.3f of the fp32 form\n", name, ms, ms * 1000.0 / TILES, ms / cal_ms * 65536.0, ms / ref_ms);
  return ms;
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
  CK(hipMalloc(&g_rows, (size_t)g_grid * 4 * ROW_SLOTS * 32 * 256 * 4));
  CK(hipMalloc(&g_bias, 512 * 4));
  CK(hipMalloc(&g_bits, (size_t)g_grid * 4 * ROW_SLOTS * 256 * 4 + 4096));
  if (!check_forms(true, w32, w16, x0, out) || !check_forms(false, w32, w16, x0, out)) { printf("check FAILED\n"); return 1; }
  if (!check_fwd(w32, w16, x0, out)) { printf("check FAILED\n"); return 1; }
  std::vector<float> h(4ull * SEG_F32);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3f * (float)((i * 2654435761u) % 2001) - 1.0f;
  CK(hipMemcpy(w32, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  // the three pieces of the same weights in hT_x's layout (split_elem, rsn_pack.hip)
  std::vector<unsigned short> hb(4ull * SEG_B16 * 2);
  for (int c = 0; c < 4; ++c) pack_pieces(h.data() + (size_t)c * SEG_F32, hb.data() + (size_t)c * SEG_B16 * 2);
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
  const double d0 = run<5, false>("(d) nine products, packed pieces, 16x16x32", w32, w16, x0, out, cal, a0);
  const double b2 = run<1, false>("(b) again", w32, w16, x0, out, cal, a0);
  const double d1 = run<5, false>("(d) again", w32, w16, x0, out, cal, a0);
  run<6, false>("(e) nine products, pieces in registers, 16x16x32", w32, w16, x0, out, cal, a0);
  run<2, false>("(c) again", w32, w16, x0, out, cal, a0);
  run<6, false>("(e) again", w32, w16, x0, out, cal, a0);
  // six of the nine products (the analytic-normal sweep's GEMMs): against (d), same run
  const double d2 = run<5, false>("(d) again", w32, w16, x0, out, cal, a0);
  const double s0 = run<10, false>("(d6) six products, packed pieces, 16x16x32", w32, w16, x0, out, cal, a0);
  const double d3 = run<5, false>("(d) again", w32, w16, x0, out, cal, a0);
  const double s1 = run<10, false>("(d6) again", w32, w16, x0, out, cal, a0);
  run<12, false>("(e6) six products, pieces in registers, 16x16x32", w32, w16, x0, out, cal, a0);
  printf("six-product go / no-go, normal sweep: (d6) / (d) wall time = %.3f (go at <= 0.850): %s\n", (s0 + s1) / (d2 + d3),
         (s0 + s1) / (d2 + d3) <= 0.85 ? "GO" : "NO-GO");
  // the backward sweep: every GEMM also keeps the 32 KiB of rows it reads (or, from the epilogue, writes) in a [points, 256] buffer
  printf("-- the backward sweep's case: the GEMM keeps its rows (32 KiB per tile to a 512 MiB buffer), the four waves on the same segment\n");
  const double f0 = run<8, false>("(a) fp32 + row stores in the K loop (gemm_run2 saver)", w32, w16, x0, out, cal, a0);
  const double g0 = run<7, false>("(d) 16x16x32 + row stores in the K loop (saver)", w32, w16, x0, out, cal, a0);
  const double h0 = run<9, false>("(d) 16x16x32 + row stores from the epilogue", w32, w16, x0, out, cal, a0);
  const double f1 = run<8, false>("(a) + stores in the loop, again", w32, w16, x0, out, cal, a0);
  const double g1 = run<7, false>("(d) + stores in the loop, again", w32, w16, x0, out, cal, a0);
  const double h1 = run<9, false>("(d) + stores from the epilogue, again", w32, w16, x0, out, cal, a0);
  {
    // six of the nine products with the row stores in the K loop (the backward sweep's stage 4): against (d) with its stores
    const double g2 = run<7, false>("(d) + stores in the loop, again", w32, w16, x0, out, cal, a0);
    const double t0 = run<11, false>("(d6) six products + row stores in the K loop", w32, w16, x0, out, cal, a0);
    const double g3 = run<7, false>("(d) + stores in the loop, again", w32, w16, x0, out, cal, a0);
    const double t1 = run<11, false>("(d6) + stores in the loop, again", w32, w16, x0, out, cal, a0);
    printf("six-product go / no-go, backward sweep: (d6) / (d), both with their stores, wall time = %.3f (go at <= 0.850): %s\n",
           (t0 + t1) / (g2 + g3), (t0 + t1) / (g2 + g3) <= 0.85 ? "GO" : "NO-GO");
  }
  {
    const double best = (g0 + g1) < (h0 + h1) ? (g0 + g1) : (h0 + h1), r = best / (f0 + f1);
    // predicted step gain, the forward's arithmetic: saving per tile and GEMM x 7 GEMMs x 16 tiles per wave and 524,288 points x 2.54
    // such launches' worth of points per step (1.33 M) x the 0.65 in-kernel yield measured on the forward
    const double gain = ((f0 + f1) - best) / 2.0 / TILES * 7.0 * 16.0 * 2.54 * 0.65;
    printf("backward go / no-go: stores in the loop %.3f, from the epilogue %.3f of the fp32 loop with its stores; the better %.3f (go at <= 0.850): %s\n",
           (g0 + g1) / (f0 + f1), (h0 + h1) / (f0 + f1), r, r <= 0.85 ? "GO" : "NO-GO");
    printf("   predicted step gain: (%.2f - %.2f) us per tile x 7 GEMMs x 16 tiles x 2.54 launches x 0.65 = %.3f ms per step\n",
           (f0 + f1) / 2.0 / TILES * 1000.0, best / 2.0 / TILES * 1000.0, gain);
  }
  {
    // the training forward's trunk: weights scaled to 0.153 of the above (standard deviation sqrt(2 / 256): a ReLU layer then keeps
    // the scale of its input), small biases of both signs; every tile's relu'd result is the next tile's operand
    printf("-- the forward trunk's case: bias start, the GEMM keeps its rows, ReLU + mask words + bias restart behind it, tile feeds tile\n");
    std::vector<float> hf(SEG_F32), hbias(512);
    for (size_t i = 0; i < hf.size(); ++i) hf[i] = 0.153f * h[i];
    for (int r = 0; r < 512; ++r) hbias[r] = 0.02f * (float)((r * 5) % 7 - 2);
    std::vector<unsigned short> hfb((size_t)SEG_B16 * 2);
    pack_pieces(hf.data(), hfb.data());
    float *w32f, *w16f;
    CK(hipMalloc(&w32f, (size_t)SEG_F32 * 4));
    CK(hipMalloc(&w16f, (size_t)SEG_B16 * 4));
    CK(hipMemcpy(w32f, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w16f, hfb.data(), hfb.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(g_bias, hbias.data(), hbias.size() * 4, hipMemcpyHostToDevice));
    const double p0 = run_fwd<0>("fp32 loop + saver, store_act_init", w32f, w16f, x0, out, cal, 0.0);
    const double q0 = run_fwd<1>("packed 16-shape + saver, store_act16_relu_init", w32f, w16f, x0, out, cal, p0);
    const double r0 = run_fwd<2>("in-register 16-shape + saver, store_act16_relu_init", w32f, w16f, x0, out, cal, p0);
    const double p1 = run_fwd<0>("fp32 loop, again", w32f, w16f, x0, out, cal, p0);
    const double q1 = run_fwd<1>("packed 16-shape, again", w32f, w16f, x0, out, cal, p0);
    const double r1 = run_fwd<2>("in-register 16-shape, again", w32f, w16f, x0, out, cal, p0);
    const double ratio = (q0 + q1) / (p0 + p1);
    printf("forward go / no-go: packed %.3f, in-register %.3f of the fp32 form (go at packed <= 0.850): %s\n", ratio, (r0 + r1) / (p0 + p1),
           ratio <= 0.85 ? "GO" : "NO-GO");
    printf("   predicted step gain: (%.2f - %.2f) us per tile x 7 GEMMs x 16 tiles x 2.54 launches x 0.65 = %.3f ms per step\n",
           (p0 + p1) / 2.0 / TILES * 1000.0, (q0 + q1) / 2.0 / TILES * 1000.0, ((p0 + p1) - (q0 + q1)) / 2.0 / TILES * 7.0 * 16.0 * 2.54 * 0.65);
  }
  printf("-- every wave on its own copy of the segment (no L1 sharing between the waves)\n");
  const double a2 = run<0, true>("(a) fp32: gemm<8, 8, PF2>", w32, w16, x0, out, cal, 0.0);
  run<1, true>("(b) nine products, packed pieces (gemm_bf16 FULL)", w32, w16, x0, out, cal, a2);
  run<2, true>("(c) nine products, pieces in registers (gemm_f32_x9)", w32, w16, x0, out, cal, a2);
  run<4, true>("    six products (gemm_bf16<8, 3>)", w32, w16, x0, out, cal, a2);
  run<5, true>("(d) nine products, packed pieces, 16x16x32", w32, w16, x0, out, cal, a2);
  run<6, true>("(e) nine products, pieces in registers, 16x16x32", w32, w16, x0, out, cal, a2);
  const double ratio = (b0 + b1) / (a0 + a1);
  printf("go / no-go: (b) / (a) wall time = %.3f (go at <= 0.850): %s\n", ratio, ratio <= 0.85 ? "GO" : "NO-GO");
  // the 16x16x32 shape: predicted step gain = (t_b - t_d) per tile x 7 GEMM equivalents x 16 tiles x 2 launches x 0.65 (the part of
  // its prediction that the nine-product change realised, profiles/normals_x9.json)
  const double gain_ms = ((b1 + b2) - (d0 + d1)) / 2.0 / TILES * 7.0 * 16.0 * 2.0 * 0.65;
  printf("shape go / no-go: (d) / (b) wall time = %.3f, predicted step gain %.3f ms (go at >= 0.300): %s\n", (d0 + d1) / (b1 + b2), gain_ms,
         gain_ms >= 0.3 ? "GO" : "NO-GO");
  return 0;
}
