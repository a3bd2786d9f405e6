// Weight packing: torch.nn.Linear layout -> the fragment order of v_mfma_f32_32x32x2_f32.
//
// Data layout in HBM (see DESIGN.md "Packed weights"): one flat fp32 buffer; every segment is
// [it][nb][lane][4] so that a wave streams it with 1 KiB-contiguous global_load_dwordx4's.
// The K index is a free permutation (it only changes the summation order); it is chosen so that the
// accumulator registers a lane holds after one layer are exactly the B-operand values the same
// lane needs for the next layer (no cross-lane movement between layers, rsn_field.hip).
// Host side: the slot maps (each once), the fillers of a job's tables, build_jobs (a network's job list) and its two runners.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "rsn_common.h"

static thread_local std::string g_last_error;

void rsn_set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

extern "C" const char* rsn_last_error(void) { return g_last_error.c_str(); }

// CU count of the CURRENT device (256 on MI355X), cached per device ordinal: a process may drive several devices.
int rsn_device_cus() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    int n = 0;
    cache[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cache[dev];
}

extern "C" int rsn_abi_version(void) { return RSN_ABI_VERSION; }

int rsn_compute_layout(const rsn_field_desc* d, RsnPackedLayout* L) {
  RSN_REQUIRE(d != nullptr, RSN_ERR_INVALID_ARGUMENT, "desc is NULL");
  RSN_REQUIRE(d->num_layers >= 1 && d->num_layers <= RSN_MAX_TRUNK_LAYERS, RSN_ERR_INVALID_ARGUMENT,
              "num_layers=%d out of range [1,%d]", d->num_layers, RSN_MAX_TRUNK_LAYERS);
  RSN_REQUIRE(d->width == 64 || d->width == 128 || d->width == 256, RSN_ERR_UNSUPPORTED,
              "width=%d unsupported (64, 128 or 256)", d->width);
  RSN_REQUIRE(d->mid_width == 128, RSN_ERR_UNSUPPORTED, "mid_width=%d unsupported (128)", d->mid_width);
  RSN_REQUIRE(d->param_width >= 0 && d->param_width <= d->width, RSN_ERR_INVALID_ARGUMENT,
              "param_width=%d must be 0 (= width) or 1..width=%d", d->param_width, d->width);
  RSN_REQUIRE(d->mma_mode >= RSN_MMA_F32 && d->mma_mode <= RSN_MMA_F32_FOLDED, RSN_ERR_INVALID_ARGUMENT, "mma_mode=%d",
              d->mma_mode);
  RSN_REQUIRE(d->skip_layer == -1 || (d->skip_layer >= 1 && d->skip_layer <= d->num_layers - 2),
              RSN_ERR_INVALID_ARGUMENT,
              "skip_layer=%d invalid for num_layers=%d (the reference MLP raises a shape error when the skip "
              "index is the last layer)", d->skip_layer, d->num_layers);
  memset(L, 0, sizeof(*L));
  L->nb = d->width / 32;
  L->nbm = d->mid_width / 32;
  const size_t blk = 256;  // floats per (it, nb) chunk: 64 lanes x 4
  size_t off = 0;
  const size_t x_seg = (size_t)(L->nb * 4) * L->nb * blk;
  const size_t enc_seg = (size_t)RSN_ENC_ITS * L->nb * blk;
  for (int l = 0; l < d->num_layers; ++l) {
    if (l == 0) {
      L->w_enc0 = off;
      off += enc_seg;
    } else {
      L->w_x[l] = off;
      off += x_seg;
      if (l == d->skip_layer) {
        L->w_enc_skip = off;
        off += enc_seg;
      }
    }
    L->b[l] = off;
    off += (size_t)d->width;
  }
  L->w_bh = off;
  off += (size_t)(L->nb * 4) * (L->nb + 1) * blk;
  L->b_bh = off;
  off += (size_t)(L->nb + 1) * 32;
  L->w_mid_sh = off;
  off += (size_t)RSN_SH_ITS * L->nbm * blk;
  L->w_mid_x = off;
  off += (size_t)(L->nb * 4) * L->nbm * blk;
  L->b_mid = off;
  off += (size_t)d->mid_width;
  L->w_rgb = off;
  off += (size_t)(L->nbm * 4) * 1 * blk;
  L->b_rgb = off;
  off += 32;
  // transposed segments
  for (int l = 1; l < d->num_layers; ++l) {
    L->wT_x[l] = off;
    off += x_seg;
  }
  const size_t encT_seg = (size_t)(L->nb * 4) * 4 * blk;  // K = W, 4 row blocks (128 >= 104 slots)
  L->wT_enc0 = off;
  off += encT_seg;
  L->wT_enc_skip = off;
  off += (d->skip_layer >= 1) ? encT_seg : 0;
  L->wT_bh = off;
  off += (size_t)(L->nb * 4 + 4) * L->nb * blk;
  L->wT_mid_x = off;
  off += (size_t)(L->nbm * 4) * L->nb * blk;
  L->wT_rgb = off;
  off += (size_t)4 * L->nbm * blk;
  L->v_density = off;
  off += (size_t)d->width;
  // split-bf16 forward segments: n_k16 * nbo * 3 chunks of 256 floats
  const size_t hx_seg = (size_t)(L->nb * 2) * L->nb * 3 * blk;
  const size_t henc_seg = (size_t)RSN_ENC_K16 * L->nb * 3 * blk;
  L->h_enc0 = off;
  off += henc_seg;
  for (int l = 1; l < d->num_layers; ++l) {
    L->h_x[l] = off;
    off += hx_seg;
  }
  L->h_enc_skip = off;
  off += (d->skip_layer >= 1) ? henc_seg : 0;
  L->h_bh = off;
  off += (size_t)(L->nb * 2) * (L->nb + 1) * 3 * blk;
  L->h_mid_sh = off;
  off += (size_t)RSN_SH_K16 * L->nbm * 3 * blk;
  L->h_mid_x = off;
  off += (size_t)(L->nb * 2) * L->nbm * 3 * blk;
  L->h_rgb = off;
  off += (size_t)(L->nbm * 2) * 1 * 3 * blk;
  for (int l = 1; l < d->num_layers; ++l) {
    L->hT_x[l] = off;
    off += hx_seg;
  }
  const size_t hencT_seg = (size_t)(L->nb * 2) * 4 * 3 * blk;
  L->hT_enc0 = off;
  off += hencT_seg;
  L->hT_enc_skip = off;
  off += (d->skip_layer >= 1) ? hencT_seg : 0;
  L->hT_bh = off;
  off += (size_t)(L->nb * 2 + 2) * L->nb * 3 * blk;
  L->hT_mid_x = off;
  off += (size_t)(L->nbm * 2) * L->nb * 3 * blk;
  L->hT_rgb = off;
  off += (size_t)2 * L->nbm * 3 * blk;
  // the seed of the analytic-normal sweep in a slot RSN_MMA_F32_FOLDED leaves unused (see RsnPackedLayout)
  L->hT_seed = (d->mma_mode == RSN_MMA_F32_FOLDED && d->num_layers >= 2) ? L->hT_x[d->num_layers - 1] : 0;
  L->hT_last = (d->mma_mode == RSN_MMA_F32_FOLDED && d->num_layers >= 2) ? (unsigned)L->hT_bh : 0u;  // pieces of wT_x[L-1] (see RsnPackedLayout)
  L->q_pf = 1;
  if ((d->mma_mode == RSN_MMA_BF16 || d->mma_mode == RSN_MMA_BF16X6) && d->width == 256) {
    // 16x32 fragments: enc 4 x 16, x 8 x 16, heads 8 x 2, bottleneck 8 x 16, mid SH 2 x 8, mid x 8 x 8, rgb 4 x 4; split-bf16:
    // three pieces per fragment (q_pf), every count below in 16 KiB groups of PIECES
    const int pf = d->mma_mode == RSN_MMA_BF16X6 ? 3 : 1;
    L->q_pf = pf;
    L->q_groups = pf * ((64 * (d->skip_layer >= 1 ? 2 : 1) + (d->num_layers - 1) * 128 + 16 + 128 + 16 + 64 + 16) / 16);
    L->q_stream = off;
    off += (size_t)L->q_groups * 16 * blk;
    // transposed fragments of the training sweeps, directly behind (see RsnPackedLayout)
    int tg = L->q_groups;
    L->t_g_begin = tg;
    tg += pf * (1 + 4 + 9);
    L->t_g_trunk = tg;
    L->t_g_encskip = -1;
    for (int l = d->num_layers - 1; l >= 1; --l) {
      if (l == d->skip_layer) { L->t_g_encskip = tg; tg += pf * 4; }
      tg += pf * 8;
    }
    L->t_g_enc0 = tg;
    tg += pf * 4;
    L->t_g_end = tg;
    off += (size_t)(tg - L->q_groups) * 16 * blk;
  }
  if (d->mma_mode == RSN_MMA_F32_FOLDED) {  // appended: every offset above is the RSN_MMA_F32 one
    const size_t pw = (size_t)(d->param_width > 0 ? d->param_width : d->width);
    L->fold_wc = off;
    off += ((size_t)d->mid_width * pw + 3) / 4 * 4;
    L->fold_bc = off;
    off += (size_t)d->mid_width;
    L->w_fold = off;
    off += (size_t)(L->nb * 4) * (L->nbm + 1) * blk;
    L->b_fold = off;
    off += (size_t)(L->nbm + 1) * 32;
    L->wT_fold = off;
    off += (size_t)(L->nbm * 4 + 4) * L->nb * blk;
  }
  L->total = off;
  return RSN_OK;
}

// ---- slot maps: where each input of a GEMM sits in the K order of its packed segment, each stated once -----------------
// Every filler below, rsn_train_saved_layout (the scatter of the weight gradients) and, independently, the host tables
// of train_graph.py (held against the library by tests/test_abi_cpu.py) are views of these functions.
namespace {
// Reference column (NeRFEncoding order: SURVEY §8(a) N2) of the u-th encoded input of a lane that owns the nf
// frequencies f0 .. f0 + nf - 1 of every coordinate, -1 for padding:
//   u in [0, 3 nf):        exp*sin of (coord c = u / nf, freq f = f0 + u % nf)  -> column c*16 + f
//   u in [3 nf, 6 nf):     exp*sin(. + pi/2) of the same                        -> column 48 + c*16 + f
//   u in [6 nf, 6 nf + 3): raw coordinate c (the lane with f0 == 0 only)        -> column 96 + c
int enc_column(int u, int f0, int nf) {
  if (u < 3 * nf) return (u / nf) * 16 + f0 + u % nf;
  if (u < 6 * nf) return 48 + ((u - 3 * nf) / nf) * 16 + f0 + u % nf;
  return (u < 6 * nf + 3 && f0 == 0) ? 96 + (u - 6 * nf) : -1;
}
// SH component of the u-th SH input of a lane that owns the n components first .. first + n - 1
int sh_column(int u, int first, int n) { return (u < n && first + u < RSN_SH_DIM) ? first + u : -1; }

// 32x32x2 kernels: slot k = it*8 + 4h + s is input u = 4 it + s of lane half h, which owns frequencies 8h .. 8h+7
// (104 slots) and SH components 17h .. 17h+16 (40 slots).  Slots past those counts map to -1 like the padding inside.
int enc_slot_to_column(int k) { return enc_column((k >> 3) * 4 + (k & 3), 8 * ((k >> 2) & 1), 8); }
int sh_slot_to_column(int k) { return sh_column((k >> 3) * 4 + (k & 3), 17 * ((k >> 2) & 1), 17); }
// ring kernels (16x32 fragments): slot k = 32 kk + 8 g + e is input u = 8 kk + e of lane group g, which owns frequencies
// 4g .. 4g+3 (128 slots) and SH components 9g .. 9g+8, 7 of them for g == 3 (64 slots)
int enc16_slot_to_column(int k) { return enc_column((k >> 5) * 8 + (k & 7), 4 * ((k >> 3) & 3), 4); }
int sh16_slot_to_column(int k) { return sh_column((k >> 5) * 8 + (k & 7), 9 * ((k >> 3) & 3), 9); }

// 16x32 fragments: output rows of every GEMM whose result feeds another GEMM are PERMUTED.  Packed row n = 16 b + 4 g + r
// (what lane group g holds in accumulator register r of block b after the MFMA) carries feature 32 (b / 2) + 8 g +
// 4 (b % 2) + r.  The eight values lane (m, g) holds of blocks 2kk, 2kk+1 are then the CONTIGUOUS features 32 kk + 8 g .. + 7:
// the K order of the next layer is the natural one (slot (kk, g, e) <- feature 32 kk + 8 g + e, lane-local hand-off as
// before), and a training kernel stores a lane's share of an activation row as ONE 16-byte piece per K-step (the four
// lanes of a point cover 64 contiguous bytes) instead of two 8-byte pieces 32 bytes apart.
int perm16_row_to_feature(int n) {
  const int b = n >> 4, g = (n >> 2) & 3, r = n & 3;
  return 32 * (b >> 1) + 8 * g + 4 * (b & 1) + r;
}

// The heads block: rows where the epilogue wants the MFMA C rows.  head: 0 density, 1 normals, 2 diff, 3 roughness, 4 tint
struct HeadRows { int head, row0, n_rows; };
constexpr HeadRows kHeads[5] = {{0, 0, 1}, {1, 1, 3}, {2, 4, 3}, {3, 8, 1}, {4, 12, 3}};
}  // namespace

extern "C" int rsn_train_saved_layout(const rsn_field_desc* d, int32_t* enc_cols, int32_t* sh_cols, int32_t* narrow_bf16,
                                      int32_t* enc_map, int32_t* sh_map) {
  RSN_REQUIRE(d && enc_cols && sh_cols && narrow_bf16 && enc_map && sh_map, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  RsnPackedLayout L;
  const int rc = rsn_compute_layout(d, &L);
  if (rc != RSN_OK) return rc;
  const bool ring = rsn_ring_training(d);  // rsn_field_bf16_train.hip / rsn_field_x6_train.hip: rows in the ring's slot order
  *enc_cols = ring ? 128 : RSN_K_ENC_PAD; *sh_cols = ring ? 64 : RSN_K_SH_PAD;
  *narrow_bf16 = (ring && d->mma_mode == RSN_MMA_BF16) ? 1 : 0;  // split-bf16: fp32 rows
  for (int s = 0; s < 128; ++s) enc_map[s] = ring ? enc16_slot_to_column(s) : enc_slot_to_column(s);
  for (int s = 0; s < 64; ++s) sh_map[s] = ring ? sh16_slot_to_column(s) : sh_slot_to_column(s);
  return RSN_OK;
}

extern "C" size_t rsn_packed_weights_bytes(const rsn_field_desc* desc) {
  RsnPackedLayout L;
  if (rsn_compute_layout(desc, &L) != RSN_OK) return 0;
  return L.total * sizeof(float);
}

// ---- one pack job = one segment -------------------------------------------------------------------
#define PACK_MAX_ROWS 288
#define PACK_MAX_COLS 256
#define PACK_MAX_SRC 6

struct PackJob {
  const float* src[PACK_MAX_SRC];
  int ld[PACK_MAX_SRC];
  float* dst;
  int n_it, nbo, is_bias, n_rows, transpose;  // transpose: packed row n <- source COLUMN, packed k <- source ROW
  int layout;  // 0: fp32 [it][nb][lane][4] (32x32x2 fragments);  1: bf16 [k32][b16][lane][8] (16x16x32 fragments)
  int16_t row_src[PACK_MAX_ROWS];  // which src a packed row comes from, -1 = zero row
  int16_t row_idx[PACK_MAX_ROWS];  // row inside that src
  int16_t col[PACK_MAX_COLS];      // source column of packed k, -1 = zero
  int16_t col_src[PACK_MAX_COLS];  // transpose == 3: which src packed k comes from (its row col[k]), -1 = zero
};

__device__ __forceinline__ void pack_elem(const PackJob& job, int e) {
  if (job.layout >= 1) {  // one bf16 of a 16x32 fragment: row 16 b + (lane & 15), k = 32 kk + 8 (lane >> 4) + el
    if (e >= job.n_it * job.nbo * 512) return;
    const int el = e & 7, lane = (e >> 3) & 63, frag = e >> 9;
    const int b = frag % job.nbo, kk = frag / job.nbo;
    const int n = b * 16 + (lane & 15), k = kk * 32 + (lane >> 4) * 8 + el;
    const int rs = job.row_src[n], c = job.col[k];
    float v = 0.0f;
    if (job.transpose == 3) {  // transposed, the SOURCE tensor selected by k ([heads]^T)
      const int cs = job.col_src[k];
      if (rs >= 0 && c >= 0 && cs >= 0) v = job.src[cs][(size_t)c * job.ld[cs] + job.row_idx[n]];
    } else if (rs >= 0 && c >= 0) {
      v = job.transpose ? job.src[rs][(size_t)c * job.ld[rs] + job.row_idx[n]]
                        : job.src[rs][(size_t)job.row_idx[n] * job.ld[rs] + c];
    }
    if (job.layout == 2) {  // split-bf16: the fragment as three pieces -- lo, mid, hi parts of v (v = hi + mid + lo up to 2^-24)
      const __bf16 b1 = (__bf16)v;
      const float r1 = v - (float)b1;
      const __bf16 b2 = (__bf16)r1;
      const __bf16 b3 = (__bf16)(r1 - (float)b2);
      __bf16* d3 = reinterpret_cast<__bf16*>(job.dst) + (size_t)frag * 1536 + (e & 511);
      d3[0] = b3; d3[512] = b2; d3[1024] = b1;
      return;
    }
    reinterpret_cast<__bf16*>(job.dst)[e] = (__bf16)v;
    return;
  }
  if (job.is_bias) {
    if (e < job.n_rows) {
      const int rs = job.row_src[e];
      job.dst[e] = rs >= 0 ? job.src[rs][job.row_idx[e]] : 0.0f;
    }
    return;
  }
  const int total = job.n_it * job.nbo * 256;
  if (e >= total) return;
  const int s = e & 3;
  const int lane = (e >> 2) & 63;
  const int chunk = e >> 8;
  const int nb = chunk % job.nbo;
  const int it = chunk / job.nbo;
  const int n = nb * 32 + (lane & 31);
  const int k = it * 8 + 4 * (lane >> 5) + s;
  const int rs = job.row_src[n];
  const int c = job.col[k];
  float v = 0.0f;
  if (job.transpose == 3) {  // transposed, the SOURCE tensor selected by k ([heads]^T: one small tensor per head)
    const int cs = job.col_src[k];
    if (rs >= 0 && c >= 0 && cs >= 0) v = job.src[cs][(size_t)c * job.ld[cs] + job.row_idx[n]];
    job.dst[e] = v;
    return;
  }
  if (rs >= 0 && c >= 0)
    v = job.transpose ? job.src[rs][(size_t)c * job.ld[rs] + job.row_idx[n]]
                      : job.src[rs][(size_t)job.row_idx[n] * job.ld[rs] + c];
  job.dst[e] = v;
}

__global__ void rsn_pack_kernel(const PackJob job) { pack_elem(job, blockIdx.x * blockDim.x + threadIdx.x); }

// Every segment in ONE launch (rsn_pack_weights_table): the job descriptors live in device memory, uploaded once per
// (parameter pointers, shape); workgroup b serves job j with block_start[j] <= b < block_start[j + 1].
// build_jobs adds 5 L + 4 s + 21 jobs at most (L trunk layers, s = 1 with a live skip; the ring stream of a bf16 mode at width 256
// included, which rsn_compute_layout lays out at every depth): 105 at RSN_MAX_TRUNK_LAYERS; a table of 96 refused 15 layers with a skip and 16 layers
#define PACK_MAX_JOBS (5 * RSN_MAX_TRUNK_LAYERS + 4 + 21 + 7)
struct PackTable {
  int n_jobs, n_blocks;
  int block_start[PACK_MAX_JOBS + 1];
  PackJob jobs[PACK_MAX_JOBS];
};

__global__ void rsn_pack_all_kernel(const PackTable* __restrict__ t) {
  const int b = blockIdx.x;
  int lo = 0, hi = t->n_jobs - 1;
  while (lo < hi) {  // last job whose first block is <= b
    const int mid = (lo + hi + 1) >> 1;
    if (t->block_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  pack_elem(t->jobs[lo], (b - t->block_start[lo]) * 256 + (int)threadIdx.x);
}

// RSN_MMA_F32_FOLDED: field_output_bottleneck folded into the x part of mlp_mid.layers.0.  Thread e < n_mid * w forms one element
// of W_c = W_mx W_b (W_mx = mid_w[:, 34:], row stride 34 + w), the next n_mid threads one element of b_c = b_mid + W_mx b_b:
// fp64 products and sums in ascending k, ONE rounding to fp32.  The results are dense tensors inside the packed buffer; the
// pack jobs of the folded segments read them as they read a parameter, so this launch goes first on the stream.
__global__ void rsn_fold_kernel(const float* __restrict__ mid_w, const float* __restrict__ mid_b, const float* __restrict__ bott_w,
                                const float* __restrict__ bott_b, int w, int n_mid, float* __restrict__ wc, float* __restrict__ bc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int ld = RSN_SH_DIM + w;
  if (e < n_mid * w) {
    const int i = e / w, j = e - i * w;
    const float* row = mid_w + (size_t)i * ld + RSN_SH_DIM;
    double acc = 0.0;
    for (int k = 0; k < w; ++k) acc += (double)row[k] * (double)bott_w[(size_t)k * w + j];
    wc[e] = (float)acc;
  } else if (e < n_mid * w + n_mid) {
    const int i = e - n_mid * w;
    const float* row = mid_w + (size_t)i * ld + RSN_SH_DIM;
    double acc = (double)mid_b[i];
    for (int k = 0; k < w; ++k) acc += (double)row[k] * (double)bott_b[k];
    bc[i] = (float)acc;
  }
}

// all split-bf16 copies in one launch
#define SPLIT_MAX_SEGS 48
struct SplitSeg { unsigned src, dst; short n_it, nbo; int block0; unsigned kscale; };  // kscale: see split_elem (0 = none)
struct SplitJob { float* packed; int n_segs; SplitSeg s[SPLIT_MAX_SEGS]; };

// split-bf16 copy of an already packed fp32 segment [it][nb][lane][4] -> [k16][nb][split(3)][lane][8 bf16]:
// element e of K=16 step kk is the fp32 value of K-iteration 2kk + (e>>2), component e&3 (zero beyond n_it), split
// EXACTLY into three bf16 (v = b1 + b2 + b3 up to 2^-24): the K=16 MFMA step consumes the same lane-local
// activations as the two fp32 K-iterations it replaces.  Works for forward and transposed segments alike.
// kscale (optional): one fp32 factor per K slot, it * 8 + 4 h + s -- the value split is rsn_seed_product(v, kscale[k]), the fp32
// product with ONE rounding.  hT_seed: wT_x[L-1] times the density row.
__device__ __forceinline__ void split_elem(const float* __restrict__ src, int n_it, int nbo, float* dstf, int e,
                                           const float* __restrict__ kscale = nullptr) {
  const int n_k16 = (n_it + 1) / 2;
  if (e >= n_k16 * nbo * 512) return;
  const int ee = e & 7;
  const int lane = (e >> 3) & 63;
  const int chunk = e >> 9;
  const int nb = chunk % nbo;
  const int kk = chunk / nbo;
  const int it = 2 * kk + (ee >> 2);
  float v = 0.0f;
  if (it < n_it) v = src[((size_t)(it * nbo + nb) * 64 + lane) * 4 + (ee & 3)];
  if (kscale != nullptr && it < n_it) v = rsn_seed_product(v, kscale[it * 8 + 4 * (lane >> 5) + (ee & 3)]);
  const __bf16 b1 = (__bf16)v;
  const float r1 = v - (float)b1;
  const __bf16 b2 = (__bf16)r1;
  const float r2 = r1 - (float)b2;
  const __bf16 b3 = (__bf16)r2;
  __bf16* dst = reinterpret_cast<__bf16*>(dstf);
  const size_t base = (size_t)(kk * nbo + nb) * 3;
  dst[((base + 0) * 64 + lane) * 8 + ee] = b1;
  dst[((base + 1) * 64 + lane) * 8 + ee] = b2;
  dst[((base + 2) * 64 + lane) * 8 + ee] = b3;
}

__global__ void rsn_pack_split_kernel(const float* __restrict__ src, int n_it, int nbo, float* dstf, const float* __restrict__ kscale) {
  split_elem(src, n_it, nbo, dstf, blockIdx.x * blockDim.x + threadIdx.x, kscale);
}

__global__ void rsn_pack_split_all_kernel(const SplitJob job) {
  int si = 0;
  while (si + 1 < job.n_segs && job.s[si + 1].block0 <= (int)blockIdx.x) ++si;
  const SplitSeg sg = job.s[si];
  split_elem(job.packed + sg.src, sg.n_it, sg.nbo, job.packed + sg.dst, ((int)blockIdx.x - sg.block0) * 256 + (int)threadIdx.x,
             sg.kscale ? job.packed + sg.kscale : nullptr);
}

namespace {

// ---- fillers of a job's row / column tables ----------------------------------------------------------------------------
// packed row n <- source row (transposed: column) index(n); a zero row where that is negative
template <class F>
void rows_from(PackJob& j, int n_rows, F index) {
  for (int n = 0; n < n_rows; ++n) {
    const int c = index(n);
    j.row_src[n] = (int16_t)(c >= 0 ? 0 : -1);
    j.row_idx[n] = (int16_t)(c >= 0 ? c : 0);
  }
}
void rows_natural(PackJob& j, int n_rows, int offset = 0) { rows_from(j, n_rows, [=](int n) { return offset + n; }); }
void cols_natural(PackJob& j, int n_cols, int offset) {
  for (int k = 0; k < n_cols; ++k) j.col[k] = (int16_t)(offset + k);
}
// packed k <- the source column a slot map gives (encoded / SH inputs)
void cols_slots(PackJob& j, int n_slots, int (*slot_to_column)(int)) {
  for (int k = 0; k < n_slots; ++k) j.col[k] = (int16_t)slot_to_column(k);
}
// 16x32 fragments: packed row n <- offset + the feature it carries; features >= n_valid (zero-padded units) are zero rows
void rows_perm16(PackJob& j, int n_rows, int n_valid, int offset = 0) {
  rows_from(j, n_rows, [=](int n) { const int f = perm16_row_to_feature(n); return f < n_valid ? offset + f : -1; });
}
// the five heads tensors (kHeads order) as sources first .. first + 4
void heads_src(PackJob& j, int first, const float* const heads[5], int ld) {
  for (int t = 0; t < 5; ++t) { j.src[first + t] = heads[t]; j.ld[first + t] = ld; }
}
// the heads block at packed rows base .. base + 15, its tensors being sources 1 .. 5 (source 0: the bottleneck)
void heads_rows(PackJob& j, int base) {
  for (const HeadRows& h : kHeads)
    for (int c = 0; c < h.n_rows; ++c) {
      j.row_src[base + h.row0 + c] = (int16_t)(1 + h.head);
      j.row_idx[base + h.row0 + c] = (int16_t)c;
    }
}
// [heads]^T (transpose = 3: k selects the source tensor, sources 0 .. 4).  Heads row hr sits at k = hr of the fp32 layout
// and, in a 16x32 fragment, at slot (g, e < 4) = k 8 g + e with hr = 4 g + e
void cols_headsT(PackJob& j, bool frag16) {
  for (const HeadRows& h : kHeads)
    for (int c = 0; c < h.n_rows; ++c) {
      const int hr = h.row0 + c, k = frag16 ? 8 * (hr >> 2) + (hr & 3) : hr;
      j.col[k] = (int16_t)c;
      j.col_src[k] = (int16_t)h.head;
    }
}
void rows_rgb(PackJob& j) {  // RGB head: rows 4..6 of its block
  for (int c = 0; c < 3; ++c) { j.row_src[4 + c] = 0; j.row_idx[4 + c] = (int16_t)c; }
}

// appends a cleared job (every row and column zero) and hands it back; the pointer holds until the next call
PackJob* add_job(std::vector<PackJob>& jobs) {
  jobs.emplace_back();
  PackJob* j = &jobs.back();
  memset(j, 0, sizeof(*j));
  for (int i = 0; i < PACK_MAX_ROWS; ++i) j->row_src[i] = -1;
  for (int i = 0; i < PACK_MAX_COLS; ++i) j->col[i] = j->col_src[i] = -1;
  return j;
}

int job_blocks(const PackJob& j) {  // workgroups of 256 threads, one element each
  return ((j.is_bias ? j.n_rows : j.n_it * j.nbo * (j.layout >= 1 ? 512 : 256)) + 255) / 256;
}
int split_blocks(const SplitSeg& s) { return (((s.n_it + 1) / 2) * s.nbo * 512 + 255) / 256; }

// Every pack job and every split-bf16 copy of one network, in launch order.  The descriptors depend on the shape and on
// the parameter / packed POINTERS only; no HIP call, no state outside the arguments.
int build_jobs(const rsn_field_desc* d, const rsn_field_params* p, float* packed, const RsnPackedLayout& L,
               std::vector<PackJob>& jobs, std::vector<SplitSeg>& splits) {
  // WP: the width the kernels run at (64 / 128 / 256); W: the width of the PARAMETER tensors (rsn_field_desc.param_width): units
  // W .. WP - 1 get zero weights and zero biases (their activations and gradients are exact zeros)
  const int WP = d->width, W = (d->param_width > 0 ? d->param_width : d->width), MW = d->mid_width, NB = L.nb, NBM = L.nbm;
  const int n_layers = d->num_layers, skip = d->skip_layer, mid_in = RSN_SH_DIM + W;  // mlp_mid: input cat([SH(34), bottleneck(W)])
  auto in_f = [&](int l) { return l == 0 ? RSN_ENC_DIM : (l == skip ? RSN_ENC_DIM + W : W); };
  auto x_off = [&](int l) { return l == skip ? RSN_ENC_DIM : 0; };  // cat([encoding, x]): x columns come second
  auto gemm = [&](const float* w, int ld, size_t dst, int n_it, int nbo, int transpose = 0) {
    PackJob* j = add_job(jobs);
    j->src[0] = w; j->ld[0] = ld; j->dst = packed + dst; j->n_it = n_it; j->nbo = nbo; j->transpose = transpose;
    return j;
  };
  auto bias = [&](const float* b, size_t dst, int n_rows) {
    PackJob* j = add_job(jobs);
    j->is_bias = 1; j->src[0] = b; j->dst = packed + dst; j->n_rows = n_rows;
    return j;
  };
  PackJob* j;  // the job being described
  for (int l = 0; l < n_layers; ++l) {
    RSN_REQUIRE(p->trunk_w[l] && p->trunk_b[l], RSN_ERR_INVALID_ARGUMENT, "trunk layer %d has NULL parameters", l);
    if (l >= 1) {
      j = gemm(p->trunk_w[l], in_f(l), L.w_x[l], NB * 4, NB);
      rows_natural(*j, W); cols_natural(*j, W, x_off(l));
    }
    if (l == 0 || l == skip) {
      j = gemm(p->trunk_w[l], in_f(l), l == 0 ? L.w_enc0 : L.w_enc_skip, RSN_ENC_ITS, NB);
      rows_natural(*j, W); cols_slots(*j, RSN_K_ENC_PAD, enc_slot_to_column);
    }
    rows_natural(*bias(p->trunk_b[l], L.b[l], WP), W);
  }

  RSN_REQUIRE(p->density_w && p->normals_w && p->roughness_w && p->diff_w && p->tint_w && p->bottleneck_w &&
                  p->mid_w && p->rgb_w && p->density_b && p->normals_b && p->roughness_b && p->diff_b &&
                  p->tint_b && p->bottleneck_b && p->mid_b && p->rgb_b,
              RSN_ERR_INVALID_ARGUMENT, "a head parameter pointer is NULL");
  const float* const heads_w[5] = {p->density_w, p->normals_w, p->diff_w, p->roughness_w, p->tint_w};
  const float* const heads_b[5] = {p->density_b, p->normals_b, p->diff_b, p->roughness_b, p->tint_b};

  j = gemm(p->bottleneck_w, W, L.w_bh, NB * 4, NB + 1);  // bottleneck (blocks 0..NB-1) + heads block NB
  heads_src(*j, 1, heads_w, W); rows_natural(*j, W); heads_rows(*j, WP); cols_natural(*j, W, 0);
  j = bias(p->bottleneck_b, L.b_bh, WP + 32);
  heads_src(*j, 1, heads_b, 0); rows_natural(*j, W); heads_rows(*j, WP);
  j = gemm(p->mid_w, mid_in, L.w_mid_sh, RSN_SH_ITS, NBM);
  rows_natural(*j, MW); cols_slots(*j, RSN_K_SH_PAD, sh_slot_to_column);
  j = gemm(p->mid_w, mid_in, L.w_mid_x, NB * 4, NBM);
  rows_natural(*j, MW); cols_natural(*j, W, RSN_SH_DIM);
  rows_natural(*bias(p->mid_b, L.b_mid, MW), MW);
  j = gemm(p->rgb_w, MW, L.w_rgb, NBM * 4, 1);  // field_output_mid (RGB head): rows 4..6 of one 32-row block
  rows_rgb(*j); cols_natural(*j, MW, 0);
  rows_rgb(*bias(p->rgb_b, L.b_rgb, 32));

  // ---------------- transposed segments (dX sweeps of the training path) ----------------
  // With transpose=1 a packed ROW selects a source COLUMN (row_idx) and a packed k selects a source ROW (col).
  for (int l = 1; l < n_layers; ++l) {
    j = gemm(p->trunk_w[l], in_f(l), L.wT_x[l], NB * 4, NB, 1);
    rows_natural(*j, W, x_off(l)); cols_natural(*j, W, 0);
  }
  for (int l : {0, skip}) {  // (encoded-input part)^T: rows = the 104 slots padded to 128
    if (l < 0) continue;
    j = gemm(p->trunk_w[l], in_f(l), l == 0 ? L.wT_enc0 : L.wT_enc_skip, NB * 4, 4, 1);
    rows_from(*j, 128, enc_slot_to_column); cols_natural(*j, W, 0);
  }
  // [bottleneck; heads]^T : rows = W input features; k < W -> bottleneck row k; k >= W -> heads row k - W.  One source per
  // job row is not enough here (k selects the source), so the two K ranges are packed separately
  j = gemm(p->bottleneck_w, W, L.wT_bh, NB * 4, NB, 1);
  rows_natural(*j, W); cols_natural(*j, W, 0);
  j = gemm(nullptr, 0, L.wT_bh + (size_t)(NB * 4) * NB * 256, 4, NB, 3);  // heads part: 4 K-iterations (k = 0..31 -> heads rows)
  heads_src(*j, 0, heads_w, W); rows_natural(*j, W); cols_headsT(*j, false);
  j = gemm(p->mid_w, mid_in, L.wT_mid_x, NBM * 4, NB, 1);  // (mlp_mid bottleneck part)^T: rows = W (source columns 34..34+W), K = mid rows
  rows_natural(*j, W, RSN_SH_DIM); cols_natural(*j, MW, 0);
  j = gemm(p->rgb_w, MW, L.wT_rgb, 4, NBM, 1);  // (RGB head)^T: rows = mid features, K = 32 with k = 4..6 -> rgb rows 0..2
  rows_natural(*j, MW);
  for (int c = 0; c < 3; ++c) j->col[4 + c] = (int16_t)c;
  rows_natural(*bias(p->density_w, L.v_density, WP), W);  // the density head's weight row, packed like a bias

  // ---------------- 16x32 bf16 fragment stream (rsn_field_bf16_ring16_kernel), straight from the nn.Linear tensors ------
  if (L.q_stream != 0) {
    int frag = 0;
    auto ring = [&](const float* w, int ld, int ks, int nbo16, int transpose = 0) {  // the stream's next ks x nbo16 fragments
      PackJob* q = gemm(w, ld, L.q_stream + (size_t)frag * 256 * L.q_pf, ks, nbo16, transpose);
      q->layout = L.q_pf == 3 ? 2 : 1;
      frag += ks * nbo16;
      return q;
    };
    for (int l = 0; l < n_layers; ++l) {
      if (l >= 1) {
        j = ring(p->trunk_w[l], in_f(l), 8, 16);
        rows_perm16(*j, WP, W); cols_natural(*j, W, x_off(l));
      }
      if (l == 0 || l == skip) {
        j = ring(p->trunk_w[l], in_f(l), 4, 16);
        rows_perm16(*j, WP, W); cols_slots(*j, 128, enc16_slot_to_column);
      }
    }
    j = ring(nullptr, W, 8, 2);  // heads: ONE 16-row block + a zero block
    heads_src(*j, 1, heads_w, W); heads_rows(*j, 0); cols_natural(*j, W, 0);
    j = ring(p->bottleneck_w, W, 8, 16);
    rows_perm16(*j, WP, W); cols_natural(*j, W, 0);
    j = ring(p->mid_w, mid_in, 2, 8);
    rows_perm16(*j, MW, MW); cols_slots(*j, 64, sh16_slot_to_column);
    j = ring(p->mid_w, mid_in, 8, 8);
    rows_perm16(*j, MW, MW); cols_natural(*j, W, RSN_SH_DIM);
    j = ring(p->rgb_w, MW, 4, 4);  // RGB head: rows 4..6 of the first of four 16-row blocks (three of them zero: whole-group padding)
    rows_rgb(*j); cols_natural(*j, MW, 0);
    RSN_REQUIRE(frag * L.q_pf == L.q_groups * 16, RSN_ERR_INVALID_ARGUMENT, "16x32 stream: %d fragments, layout says %d groups",
                frag, L.q_groups);
    // ---- transposed pieces (training sweeps): packed ROW <- the input feature it carries (source COLUMN), packed K natural
    //      <- output feature (source ROW); transpose = 1 as above
    j = ring(p->rgb_w, MW, 2, 8, 1);  // (RGB head)^T: rows = 128 hidden features; K-step 0 slot (g = 1, e = 0..2) = k 8..10 <- rgb rows; K-step 1 zero
    rows_perm16(*j, MW, MW);
    for (int c = 0; c < 3; ++c) j->col[8 + c] = (int16_t)c;
    j = ring(p->mid_w, mid_in, 4, 16, 1);  // (mlp_mid x part)^T: rows = W bottleneck features (source columns 34..), K = 128 hidden rows
    rows_perm16(*j, WP, W, RSN_SH_DIM); cols_natural(*j, MW, 0);
    j = ring(p->bottleneck_w, W, 8, 16, 1);  // [bottleneck]^T: rows = W embedding features, K = W bottleneck rows ...
    rows_perm16(*j, WP, W); cols_natural(*j, W, 0);
    j = ring(nullptr, 0, 1, 16, 3);  // ... + [heads]^T as a ninth K-step
    heads_src(*j, 0, heads_w, W); rows_perm16(*j, WP, W); cols_headsT(*j, true);
    for (int l = n_layers - 1; l >= 0; --l) {  // last: (layer 0)^T, encoded inputs only
      if (l == 0 || l == skip) {  // encoded-input slots as packed rows: row 16 b + 4 g + r is slot (kk = b / 2, g, e = 4 (b % 2) + r)
        j = ring(p->trunk_w[l], in_f(l), 8, 8, 1);
        rows_from(*j, 128, [](int n) { return enc16_slot_to_column(perm16_row_to_feature(n)); }); cols_natural(*j, W, 0);
      }
      if (l >= 1) {
        j = ring(p->trunk_w[l], in_f(l), 8, 16, 1);
        rows_perm16(*j, WP, W, x_off(l)); cols_natural(*j, W, 0);
      }
    }
    RSN_REQUIRE(frag * L.q_pf == L.t_g_end * 16, RSN_ERR_INVALID_ARGUMENT, "transposed 16x32 stream: %d fragments, layout says %d groups",
                frag, L.t_g_end);
  }

  // ---------------- RSN_MMA_F32_FOLDED: [W_c ; heads] forward and transposed, from the dense W_c / b_c of rsn_fold_kernel ------
  if (d->mma_mode == RSN_MMA_F32_FOLDED) {
    const float* wc = packed + L.fold_wc;
    j = gemm(wc, W, L.w_fold, NB * 4, NBM + 1);  // W_c (blocks 0..NBM-1) + heads block NBM: the heads rows as in w_bh
    heads_src(*j, 1, heads_w, W); rows_natural(*j, MW); heads_rows(*j, MW); cols_natural(*j, W, 0);
    j = bias(packed + L.fold_bc, L.b_fold, MW + 32);
    heads_src(*j, 1, heads_b, 0); rows_natural(*j, MW); heads_rows(*j, MW);
    j = gemm(wc, W, L.wT_fold, NBM * 4, NB, 1);  // [W_c]^T: rows = W embedding features, K = the mid rows ...
    rows_natural(*j, W); cols_natural(*j, MW, 0);
    j = gemm(nullptr, 0, L.wT_fold + (size_t)(NBM * 4) * NB * 256, 4, NB, 3);  // ... + [heads]^T as four more K-iterations (wT_bh)
    heads_src(*j, 0, heads_w, W); rows_natural(*j, W); cols_headsT(*j, false);
  }

  // ---------------- split-bf16 copies (RSN_MMA_BF16X6 / X3 / BF16) of every GEMM segment ----------------
  auto split = [&](size_t src, int n_it, int nbo, size_t dst, size_t kscale = 0) {  // block0: numbered by the single-launch path
    splits.push_back(SplitSeg{(unsigned)src, (unsigned)dst, (short)n_it, (short)nbo, 0, (unsigned)kscale});
  };
  if (d->mma_mode == RSN_MMA_F32 || d->mma_mode == RSN_MMA_F32_FOLDED) {
    // exact fp32: the forward and backward kernels read none of the copies below.  The folded mode splits what the analytic-normal
    // sweep of its training forward reads (nine-product loop, rsn_gemm_loops.h): the seed, then the transposed trunk and encoded-input
    // segments behind it, and the forward trunk segments h_x[l], which the W x W GEMMs of its training forward read the same way
    // (RSN_MMA_F32 packs nothing more: its training kernel forms the same pieces in registers)
    if (L.hT_seed != 0) split(L.wT_x[n_layers - 1], NB * 4, NB, L.hT_seed, L.v_density);
    if (d->mma_mode == RSN_MMA_F32_FOLDED) {
      for (int l = 1; l + 1 < n_layers; ++l) split(L.wT_x[l], NB * 4, NB, L.hT_x[l]);
      if (L.hT_last != 0) split(L.wT_x[n_layers - 1], NB * 4, NB, L.hT_last);  // the backward sweep's first trunk GEMM
      if (skip >= 1) split(L.wT_enc_skip, NB * 4, 4, L.hT_enc_skip);
      split(L.wT_enc0, NB * 4, 4, L.hT_enc0);
      for (int l = 1; l < n_layers; ++l) split(L.w_x[l], NB * 4, NB, L.h_x[l]);  // the training forward's trunk GEMMs
    }
    return RSN_OK;
  }
  split(L.w_enc0, RSN_ENC_ITS, NB, L.h_enc0);
  for (int l = 1; l < n_layers; ++l) {
    split(L.w_x[l], NB * 4, NB, L.h_x[l]);
    split(L.wT_x[l], NB * 4, NB, L.hT_x[l]);
  }
  if (skip >= 1) {
    split(L.w_enc_skip, RSN_ENC_ITS, NB, L.h_enc_skip);
    split(L.wT_enc_skip, NB * 4, 4, L.hT_enc_skip);
  }
  split(L.wT_enc0, NB * 4, 4, L.hT_enc0);
  split(L.w_bh, NB * 4, NB + 1, L.h_bh);
  split(L.wT_bh, NB * 4 + 4, NB, L.hT_bh);
  split(L.w_mid_sh, RSN_SH_ITS, NBM, L.h_mid_sh);
  split(L.w_mid_x, NB * 4, NBM, L.h_mid_x);
  split(L.wT_mid_x, NBM * 4, NB, L.hT_mid_x);
  split(L.w_rgb, NBM * 4, 1, L.h_rgb);
  split(L.wT_rgb, 4, NBM, L.hT_rgb);
  return RSN_OK;
}

// the job lists of the calling thread, reused across calls: packing is on the host path of every training step
thread_local std::vector<PackJob> t_jobs;
thread_local std::vector<SplitSeg> t_splits;

// what both entry points check, then the build into t_jobs / t_splits
int validate_and_build(const rsn_field_desc* d, const rsn_field_params* p, float* packed, size_t packed_bytes) {
  RsnPackedLayout L;
  const int rc = rsn_compute_layout(d, &L);
  if (rc != RSN_OK) return rc;
  RSN_REQUIRE(p != nullptr && packed != nullptr, RSN_ERR_INVALID_ARGUMENT, "params/packed is NULL");
  RSN_REQUIRE(packed_bytes >= L.total * sizeof(float), RSN_ERR_WORKSPACE,
              "packed buffer too small: %zu < %zu bytes", packed_bytes, L.total * sizeof(float));
  t_jobs.clear(); t_splits.clear();
  return build_jobs(d, p, packed, L, t_jobs, t_splits);
}

}  // namespace

// RSN_MMA_F32_FOLDED: W_c / b_c into the packed buffer, ahead of the pack jobs that read them (validate_and_build has checked p)
static int launch_fold(const rsn_field_desc* d, const rsn_field_params* p, float* packed, hipStream_t st) {
  if (d->mma_mode != RSN_MMA_F32_FOLDED) return RSN_OK;
  RsnPackedLayout L;
  RSN_TRY(rsn_compute_layout(d, &L));
  const int w = d->param_width > 0 ? d->param_width : d->width, n = d->mid_width * w + d->mid_width;
  hipLaunchKernelGGL(rsn_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->mid_w, p->mid_b, p->bottleneck_w,
                     p->bottleneck_b, w, d->mid_width, packed + L.fold_wc, packed + L.fold_bc);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

// one launch per segment, then one per split-bf16 copy
extern "C" int rsn_pack_weights(const rsn_field_desc* d, const rsn_field_params* p, float* packed,
                                size_t packed_bytes, void* stream) {
  const int rc = validate_and_build(d, p, packed, packed_bytes);
  if (rc != RSN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  RSN_TRY(launch_fold(d, p, packed, st));
  for (const PackJob& j : t_jobs) {
    hipLaunchKernelGGL(rsn_pack_kernel, dim3((unsigned)job_blocks(j)), dim3(256), 0, st, j);
    RSN_HIP(hipGetLastError());
  }
  for (const SplitSeg& s : t_splits) {
    hipLaunchKernelGGL(rsn_pack_split_kernel, dim3((unsigned)split_blocks(s)), dim3(256), 0, st, packed + s.src, (int)s.n_it,
                       (int)s.nbo, packed + s.dst, s.kscale ? packed + s.kscale : nullptr);
    RSN_HIP(hipGetLastError());
  }
  return RSN_OK;
}

// ---- the same in (at most) two launches: every fp32 segment, every split-bf16 copy ----------------
extern "C" size_t rsn_pack_table_bytes(void) { return sizeof(PackTable); }

extern "C" int rsn_pack_weights_table(const rsn_field_desc* d, const rsn_field_params* p, float* packed,
                                      size_t packed_bytes, void* table, size_t table_bytes, int32_t rebuild_table,
                                      void* stream) {
  RSN_REQUIRE(table != nullptr && table_bytes >= sizeof(PackTable), RSN_ERR_WORKSPACE,
              "job table buffer too small: %zu < %zu bytes", table_bytes, sizeof(PackTable));
  const int rc = validate_and_build(d, p, packed, packed_bytes);
  if (rc != RSN_OK) return rc;
  RSN_REQUIRE((int)t_jobs.size() <= PACK_MAX_JOBS && (int)t_splits.size() <= SPLIT_MAX_SEGS, RSN_ERR_UNSUPPORTED,
              "%zu pack jobs / %zu split segments exceed the table", t_jobs.size(), t_splits.size());
  hipStream_t st = (hipStream_t)stream;
  static thread_local PackTable host_table;  // stays alive behind the asynchronous upload
  const int n_jobs = (int)t_jobs.size();
  int blocks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    if (rebuild_table) { host_table.block_start[i] = blocks; host_table.jobs[i] = t_jobs[i]; }
    blocks += job_blocks(t_jobs[i]);
  }
  if (rebuild_table) {  // the caller says a pointer or the shape changed (or this is the first use): upload the table
    host_table.n_jobs = n_jobs;
    host_table.n_blocks = host_table.block_start[n_jobs] = blocks;
    RSN_HIP(hipMemcpyAsync(table, &host_table, sizeof(PackTable), hipMemcpyHostToDevice, st));
  }
  RSN_TRY(launch_fold(d, p, packed, st));
  hipLaunchKernelGGL(rsn_pack_all_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const PackTable*)table);
  RSN_HIP(hipGetLastError());
  if (!t_splits.empty()) {
    SplitJob sj;
    memset(&sj, 0, sizeof(sj));
    sj.packed = packed; sj.n_segs = (int)t_splits.size();
    int b = 0;
    for (int i = 0; i < sj.n_segs; ++i) {
      sj.s[i] = t_splits[i];
      sj.s[i].block0 = b;
      b += split_blocks(sj.s[i]);
    }
    hipLaunchKernelGGL(rsn_pack_split_all_kernel, dim3((unsigned)b), dim3(256), 0, st, sj);
    RSN_HIP(hipGetLastError());
  }
  return RSN_OK;
}
