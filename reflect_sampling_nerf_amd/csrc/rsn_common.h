// Shared declarations of librsn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "rsn.h"

#define RSN_K_ENC_PAD 104  // 99 encoded inputs padded to 13 K-iterations of 8
#define RSN_K_SH_PAD 40    // 34 SH inputs padded to 5 K-iterations of 8
#define RSN_ENC_ITS (RSN_K_ENC_PAD / 8)
#define RSN_SH_ITS (RSN_K_SH_PAD / 8)
#define RSN_ENC_K16 7      // encoded inputs in K=16 steps (112 >= 104)
#define RSN_SH_K16 3       // SH inputs in K=16 steps (48 >= 40)
#define RSN_AUX_ITS 6      // LDS K-iterations reserved for the SH inputs (even, for the K=16 steps)

void rsn_set_error(const char* fmt, ...);
int rsn_device_cus();                   // CU count of the current device (cached per device)

#define RSN_REQUIRE(cond, code, ...)        \
  do {                                      \
    if (!(cond)) {                          \
      rsn_set_error(__VA_ARGS__);           \
      return (code);                        \
    }                                       \
  } while (0)

#define RSN_TRY(call)                       \
  do {                                      \
    const int rc_ = (call);                 \
    if (rc_ != RSN_OK) return rc_;          \
  } while (0)

#define RSN_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      rsn_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return RSN_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)

// Offsets (in floats) of every packed segment inside the flat packed-weights buffer.
// A weight segment with n_it K-iterations and nbo 32-row output blocks is laid out
// [it][nb][lane(64)][4]: the float4 that lane (i = lane&31, h = lane>>5) feeds to the four
// v_mfma_f32_32x32x2_f32 K-steps of iteration `it` for output block nb, i.e.
// W[nb*32 + i][col(it*8 + 4h + s)], s = 0..3.
struct RsnPackedLayout {
  int nb;           // width / 32
  int nbm;          // mid_width / 32
  size_t w_x[RSN_MAX_TRUNK_LAYERS];   // x-part of layer l (l >= 1)
  size_t w_enc0;                      // layer 0 (encoding input)
  size_t w_enc_skip;                  // encoding part of the skip layer
  size_t b[RSN_MAX_TRUNK_LAYERS];     // bias of layer l
  size_t w_bh, b_bh;                  // bottleneck (nb blocks) + heads (1 block)
  size_t w_mid_sh, w_mid_x, b_mid;    // mlp_mid: SH part, bottleneck part
  size_t w_rgb, b_rgb;                // field_output_mid (rows 4..6 of one block)
  // transposed segments (training: dX sweeps).  Rows = the layer's INPUT features, K = its output features.
  size_t wT_x[RSN_MAX_TRUNK_LAYERS];  // (x-part of layer l)^T, l >= 1: rows W, K = W
  size_t wT_enc0, wT_enc_skip;        // (encoded-input part)^T: rows = 104 slots padded to 128, K = W
  size_t wT_bh;                       // [bottleneck; heads]^T: rows W, K = W + 32
  size_t wT_mid_x;                    // (bottleneck part of mlp_mid)^T: rows W, K = mid_width
  size_t wT_rgb;                      // (RGB head)^T: rows mid_width, K = 32 (k = 4..6 live)
  size_t v_density;                   // density head weight row [W] (seed of the analytic-normal sweep)
  // split-bf16 copies of the forward segments (RSN_MMA_BF16X6 / X3): [k16][nb][split(3)][lane][8 bf16];
  // offsets in floats like everything else (one (k16, nb, split) chunk = 1 KiB = 256 floats)
  size_t h_x[RSN_MAX_TRUNK_LAYERS];
  size_t h_enc0, h_enc_skip, h_bh, h_mid_sh, h_mid_x, h_rgb;
  size_t hT_x[RSN_MAX_TRUNK_LAYERS];  // split-bf16 copies of the transposed segments (training sweeps)
  size_t hT_enc0, hT_enc_skip, hT_bh, hT_mid_x, hT_rgb;
  // RSN_MMA_F32_FOLDED writes hT_x[1 .. L-2], hT_enc_skip and hT_enc0 too (and, of the other h* / hT_* regions, only hT_last
  // below and h_x[1 .. L-1]): the loop GEMMs of the analytic-normal sweep of its training forward read them with six of the nine
  // piece products (gemm_bf16_s16<.., 6>); the W x W GEMMs of its backward sweep (rsn_field_bwd.hip, stage 4) read them with all
  // nine (gemm_bf16_s16<.., 9>), as the W x W GEMMs of its training forward's trunk read h_x[l].
  // RSN_MMA_F32 writes none: its training kernel forms the same pieces from the w_x / wT_* segments in registers (gemm_f32_s16)
  // RSN_MMA_F32_FOLDED with num_layers >= 2 only (0 = absent): V = (x part of layer L-1)^T diag(w_density), one rounding per
  // element (rsn_seed_product), as three bf16 pieces in the layout and K order of hT_x[L-1] -- the first GEMM of the
  // analytic-normal sweep reads it against the ReLU bits of layer L-1 (gemm_bf16_bits).  It takes the PLACE of hT_x[L-1]: the
  // exact-fp32 modes neither write nor read their split-bf16 copies, so the folded buffer keeps its size.  The RSN_MMA_F32
  // buffer keeps every byte: its training kernel forms the same pieces from wT_x[L-1] and v_density in registers
  size_t hT_seed;
  // RSN_MMA_BF16 / BF16X6 at width 256 only: the whole network as 16x32 fragments for v_mfma_f32_16x16x32_bf16, ONE linear
  // stream in the exact order rsn_field_bf16_ring16_kernel consumes them (its workgroups pull it through an LDS ring): lane
  // (i = lane & 15, g = lane >> 4) holds W[16 b + i][feature(kk, g, e)], e = 0..7, of fragment (K-step kk, row block b)
  size_t q_stream;                    // 0 = absent
  int q_groups;
  // ... and, directly behind it (group indices continue), the TRANSPOSED 16x32 fragments of the training sweeps
  // (rsn_field_bf16_train.hip) in consumption order: (RGB head)^T 1 group, (mlp_mid x part)^T 4, [bottleneck; heads]^T 9,
  // then for l = L-1 .. 1: (encoded-input part of the skip layer)^T 4 groups in front of l == skip, (x part of layer l)^T 8;
  // last (layer 0)^T 4 groups.  The backward sweep walks all of it (without the two encoded-input pieces when no input
  // gradient is wanted); the analytic-normal sweep of the training forward walks [t_g_trunk, t_g_end) behind the forward stream.
  int t_g_begin, t_g_trunk, t_g_encskip, t_g_enc0, t_g_end;   // absolute group indices from q_stream; t_g_encskip = -1: no skip layer
  // RSN_MMA_BF16X6 at width 256 (rsn_field_x6_train.hip): the same stream with every fragment as THREE 1 KiB pieces -- the lo, mid
  // and hi bf16 parts of the fp32 weights, in that order (small products first); q_pf = 3 and every group count above is x 3
  int q_pf;                           // 1 KiB pieces per fragment of q_stream: 1 (plain bf16) or 3 (split-bf16)
  // RSN_MMA_F32_FOLDED with num_layers >= 2 only (0 = absent): the three bf16 pieces of wT_x[L-1] itself, whose place hT_seed has
  // taken, for the first trunk GEMM of the folded backward sweep (gemm_bf16_s16).  They live in the hT_bh region, which the folded
  // mode neither writes nor reads otherwise and which holds nb * 2 + 2 K = 16 steps against the nb * 2 of an hT_x segment: no offset
  // or size moves.  32 bits in the four bytes that padded q_pf (static_assert below): the struct is passed to every field kernel,
  // and this way no kernel's arguments move
  unsigned hT_last;
  // RSN_MMA_F32_FOLDED only (0 = absent), appended behind everything above: the bottleneck folded into mlp_mid's x part.
  //   fold_wc / fold_bc  W_c = W_mid[:, 34:] W_b as a dense [mid_width, param_width] tensor and b_c [mid_width] (rsn_fold_kernel
  //                      writes them, the pack jobs of the three segments below read them like parameters)
  //   w_fold / b_fold    [W_c ; heads]: K = W, nbm + 1 row blocks (the heads block last), and its bias
  //   wT_fold            [W_c ; heads]^T: rows W, K = mid_width + 32 (the K-concatenation of wT_bh)
  size_t fold_wc, fold_bc, w_fold, b_fold, wT_fold;
  size_t total;                       // floats
};
static_assert(offsetof(RsnPackedLayout, fold_wc) == offsetof(RsnPackedLayout, hT_last) + 4 &&
                  offsetof(RsnPackedLayout, hT_last) == offsetof(RsnPackedLayout, q_pf) + 4,
              "hT_last fills the padding behind q_pf");
#define RSN_RING_GROUP_FRAGS 16   // 1 KiB weight fragments per ring group
#define RSN_RING_MAX_LAYERS 10   // trunk depth the ring kernels' LDS bias table is sized for
// the TRAINING kernels on the LDS weight ring (rsn_field_bf16_train.hip: plain bf16; rsn_field_x6_train.hip: split-bf16) serve
// this shape; every other shape / mode trains on rsn_field_kernel<., true, .> / rsn_field_bwd_kernel
inline bool rsn_ring_training(const rsn_field_desc* d) {
  return (d->mma_mode == RSN_MMA_BF16 || d->mma_mode == RSN_MMA_BF16X6) && d->width == 256 &&
         d->num_layers <= RSN_RING_MAX_LAYERS;
}

int rsn_compute_layout(const rsn_field_desc* desc, RsnPackedLayout* L);

// One element of V = W_{L-1}^T diag(w_density): the fp32 product, rounded once (-ffp-contract=off).  The pack kernel (hT_seed)
// and the RSN_MMA_F32 training kernel (in registers) both form V with this function, then split it the same way: same bits.
__device__ __forceinline__ float rsn_seed_product(float w, float wd) { return w * wd; }
