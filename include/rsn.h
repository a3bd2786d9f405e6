/*
 * rsn.h -- C ABI of librsn_hip.so: the MI355X (gfx950) implementation of the
 * reflect-sampling-nerf ray-batch volume-rendering hot path.
 *
 * The reference (236088/reflect-sampling-nerf) is pure Python on PyTorch and has NO FFI for this
 * path; its boundary is the Nerfstudio Model/Field plugin surface.  This header
 * is the boundary the build introduces underneath that surface: each entry point below replaces a
 * group of reference calls, cited as file:line relative to /root/reference/reflect_sampling_nerf/.
 * The Python host mirror (reflect_sampling_nerf_amd/) binds these with ctypes; INTEGRATION.md shows
 * the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer to fp32 (or int32) unless it says host;
 *   - no allocation and no ownership transfer inside the library: the caller (torch) owns inputs,
 *     outputs and workspaces;
 *   - every call is asynchronous on the given hipStream_t (passed as void*), never synchronises
 *     the host, and is re-entrant for distinct streams;
 *   - return 0 on success, a negative rsn_status otherwise; rsn_last_error() gives the message
 *     (thread-local);
 *   - "n_dev": optional device pointer to an int32 ray count that overrides the host count at run
 *     time (dynamic number M of reflected rays, no host sync); pass NULL to use the host count.
 */
#ifndef RSN_H
#define RSN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSN_ABI_VERSION 18
#define RSN_MAX_TRUNK_LAYERS 16
#define RSN_NUM_FREQS 16   /* NeRFEncoding(num_frequencies=16), reflect_sampling_nerf_model.py:98-100 */
#define RSN_ENC_DIM 99     /* 3*16*2 + 3 */
#define RSN_SH_DIM 34      /* IntegratedSHEncoding.get_out_dim, reflect_sampling_nerf_components.py:49-50 */

typedef enum rsn_status {
  RSN_OK = 0,
  RSN_ERR_INVALID_ARGUMENT = -1,
  RSN_ERR_UNSUPPORTED = -2,
  RSN_ERR_HIP = -3,
  RSN_ERR_WORKSPACE = -4
} rsn_status;

typedef enum rsn_spacing { RSN_SPACING_UNIFORM = 0, RSN_SPACING_RECIPROCAL = 1 } rsn_spacing;

/* Shape of the Field: constructor knobs of ReflectSamplingNeRFNerfField
 * (reflect_sampling_nerf_field.py:36-47) plus the frequency table of the position encoding the
 * model builds for it (reflect_sampling_nerf_model.py:98-100: 2**linspace(0,16,16), computed by the
 * caller so that it is bit-identical to the host framework's table). */
typedef struct rsn_field_desc {
  int32_t num_layers;   /* trunk nn.Linear count (base_mlp_num_layers), 1..RSN_MAX_TRUNK_LAYERS */
  int32_t width;        /* base_mlp_layer_width: 64, 128 or 256 */
  int32_t skip_layer;   /* layer whose input is cat([encoding, x]): 1..num_layers-2 (4 when num_layers >= 6), or -1 */
  int32_t mid_width;    /* head_mlp_layer_width: 128 */
  float density_bias;   /* 0.5 */
  float freqs[RSN_NUM_FREQS];
  int32_t mma_mode;     /* arithmetic of the dense GEMMs in the eval field kernel (rsn_mma_mode) */
  int32_t param_width;  /* base_mlp_layer_width of the PARAMETER tensors when it is not one of the widths the kernels run at:
                         * any 1 <= param_width <= width; 0 = width.  The kernels run at `width` (the next of 64 / 128 / 256)
                         * with zero-padded units: rsn_pack_weights gives units param_width .. width - 1 zero weights and
                         * biases, their activations and gradients are exact zeros, every wide buffer ([N, W] rows) has
                         * `width` columns of which the first param_width are live (ABI 15) */
} rsn_field_desc;

/* How the field kernel multiplies fp32 operands on the matrix cores:
 *   RSN_MMA_F32     v_mfma_f32_32x32x2_f32: exact fp32 products (157 TFLOP/s peak); in the training forward (this mode and
 *                   RSN_MMA_F32_FOLDED) the W x W GEMMs of the trunk run as nine exact bf16 piece products and the loop GEMMs of
 *                   the analytic-normal sweep as the six largest of them (each dropped term <= 2^-25 relative); the backward
 *                   sweep of this mode is on the fp32 MFMA loop, that of RSN_MMA_F32_FOLDED runs its W x W GEMMs as the nine
 *                   products; the training graph reduces the weight gradients of such a field with RSN_MMA_BF16X6 (a call that
 *                   names RSN_MMA_F32 runs the fp32 reduction);
 *   RSN_MMA_BF16X6  fp32 emulation: both operands split exactly into 3 bf16 (8+8+8 mantissa bits), the 6 leading
 *                   cross products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (dropped terms <= 2^-24
 *                   relative): fp32-equivalent results at 6/16 of the fp32-MFMA cost;
 *   RSN_MMA_BF16X3  2-way split, 3 products (~2^-16 relative): reduced precision, opt-in only;
 *   RSN_MMA_BF16    plain bf16 operands (1 product, 8 mantissa bits), fp32 accumulate: BASELINE configs[3]
 *                   ("bf16 MFMA hidden GEMMs"); encode, heads' activations and compositing stay fp32;
 *   RSN_MMA_F32_FOLDED  RSN_MMA_F32 with field_output_bottleneck folded into the x part of mlp_mid.layers.0 in the
 *                   TRAINING kernels (two affine maps with nothing between them are one): W_c = W_mid[:, 34:] W_b,
 *                   b_c = b_mid + W_mid[:, 34:] b_b, formed with fp64 accumulation when the weights are packed.  The packed
 *                   buffer is the RSN_MMA_F32 one with the folded segments appended; rsn_field_saved.bott and
 *                   rsn_field_grads_out.d_bott are neither written nor read (NULL is fine); the parameter gradients of the
 *                   two layers come from rsn_unfold_bottleneck_grads.  Eval launches run the RSN_MMA_F32 kernels. */
typedef enum rsn_mma_mode {
  RSN_MMA_F32 = 0, RSN_MMA_BF16X6 = 1, RSN_MMA_BF16X3 = 2, RSN_MMA_BF16 = 3, RSN_MMA_F32_FOLDED = 4
} rsn_mma_mode;

/* Parameters in torch.nn.Linear layout: weight [out,in] row-major, bias [out]; names follow the
 * reference Field's state_dict (reflect_sampling_nerf_field.py:54-86).  field_output_low (:67) is
 * never evaluated by the model and is therefore absent. */
typedef struct rsn_field_params {
  const float* trunk_w[RSN_MAX_TRUNK_LAYERS]; /* mlp_base.layers.{i}.weight */
  const float* trunk_b[RSN_MAX_TRUNK_LAYERS]; /* mlp_base.layers.{i}.bias   */
  const float* density_w;    const float* density_b;    /* field_output_density.net    [1,W]      */
  const float* normals_w;    const float* normals_b;    /* field_output_normals.net    [3,W]      */
  const float* roughness_w;  const float* roughness_b;  /* field_output_roughness.net  [1,W]      */
  const float* diff_w;       const float* diff_b;       /* field_output_diff.net       [3,W]      */
  const float* tint_w;       const float* tint_b;       /* field_output_tint.net       [3,W]      */
  const float* bottleneck_w; const float* bottleneck_b; /* field_output_bottleneck.net [W,W]      */
  const float* mid_w;        const float* mid_b;        /* mlp_mid.layers.0            [mid,34+W] */
  const float* rgb_w;        const float* rgb_b;        /* field_output_mid.net        [3,mid]    */
} rsn_field_params;

/* Per-sample outputs of one field evaluation; any pointer may be NULL (output skipped). */
typedef struct rsn_field_outputs {
  float* sigma;        /* [N]    softplus(raw + density_bias)         field.py:133-136 */
  float* color;        /* [N,3]  diff + tint * mid                    model.py:175,209,310,336 */
  float* pred_normals; /* [N,3]  get_pred_normals                     field.py:139-144 */
  float* n_dot_d;      /* [N]    get_reflection's n.d                 field.py:203-204 */
  float* diff;         /* [N,3]  get_diff                             field.py:176-180 */
  float* tint;         /* [N,3]  get_tint                             field.py:182-186 */
  float* roughness;    /* [N]    sigmoid(roughness head)              field.py:150-155 (default act) */
  float* raw_density;  /* [N]    density head before bias/softplus    field.py:133-135 */
  float* raw_roughness;/* [N]    roughness head before its activation field.py:150-155 (caller-chosen act) */
} rsn_field_outputs;

/* Activations the training-mode forward keeps for the backward pass (row-major, N = n_rays*n_samples rows; W = width,
 * L = num_layers).  Written by rsn_field_forward_frustum_train.  fp32 -- except in the reduced-precision training mode
 * (rsn_field_desc.mma_mode == RSN_MMA_BF16, whose GEMMs round these values to bf16 anyway): there the three WIDE buffers
 * act, bott and hid hold bf16 (same shapes, 2 bytes per element; half the step's HBM stream), and so do the wide layer
 * gradients dy, d_bott, da_mid of rsn_field_grads_out; rsn_weight_grad_multi_dev reads them as such (operand_bf16). */
typedef struct rsn_field_saved {
  float* enc;     /* [N,104]  encoded inputs (input of trunk layer 0), kernel slot order                   */
  float* act;     /* [L,N,W]  post-ReLU output of trunk layer l (act[L-1] = embedding)                       */
  float* bott;    /* [N,W]    bottleneck output (RSN_MMA_F32_FOLDED: not touched, may be NULL)                */
  float* sh;      /* [N,40]   attenuated SH-34 inputs of mlp_mid, kernel slot order                          */
  float* hid;     /* [N,128]  mlp_mid hidden (post-ReLU)                                                     */
  float* heads;   /* [N,8]    raw normal head (3), raw roughness head (1), mid RGB (3), pad                  */
  float* normals; /* [N,3]    OUT: analytic normals -normalize(d raw_density/d mean) (field.py:146-147),     *
                   *          or NULL to skip the sweep (reflect levels, model.py:295,321)                    */
  uint32_t* relu_bits; /* [L+1,N,2,max(W/64,2)] ReLU masks (pre-activation > 0) of trunk layer l (l < L) and of the mlp_mid *
                   *          hidden layer (l = L), bit-packed per lane half: what the dX sweeps mask by            */
} rsn_field_saved;

int rsn_abi_version(void);
const char* rsn_last_error(void);

/* Layout of the two NARROW saved buffers of a training forward, which depends on the kernel that serves the Field's shape and
 * MMA mode (ABI 15).  Default (rsn_field_kernel): enc = fp32 [N,104], sh = fp32 [N,40] in that kernel's slot order.  With
 * mma_mode == RSN_MMA_BF16 at width 256 the training forward / backward run on the LDS weight ring
 * (rsn_field_bf16_train.hip): enc = bf16 [N,128], sh = bf16 [N,64], slot s = 32 kk + 8 g + e of lane group g, and the
 * ReLU bit words of rsn_field_saved.relu_bits are laid out [L+1][N][4 lane groups][2 words].  mma_mode == RSN_MMA_BF16X6 at
 * width 256 (rsn_field_x6_train.hip, the split-bf16 = fp32-equivalent mode on the same ring): the same slot order and bit
 * layout, enc / sh rows in fp32 (narrow_bf16 = 0); every wide buffer stays fp32 [N,W] in natural feature order.
 * Outputs: *enc_cols / *sh_cols = row length in elements, *narrow_bf16 = 1 if enc / sh rows hold bf16; enc_map[s] / sh_map[s]
 * (caller arrays of 128 / 64 ints, HOST) = column of the reference's 99-wide NeRFEncoding output / 34-wide SH encoding
 * (nerfstudio N2; reflect_sampling_nerf_components.py:38-140) that slot s carries, -1 for padding: the col_map of the
 * weight gradients of trunk layer 0 / the skip layer (rsn_weight_grad_jobs) and of mlp_mid's SH part. */
int rsn_train_saved_layout(const rsn_field_desc* desc, int32_t* enc_cols, int32_t* sh_cols, int32_t* narrow_bf16,
                           int32_t* enc_map, int32_t* sh_map);

/* ---- weights: nn.Linear layout -> MFMA fragment order ---------------------------------------
 * The field kernels stream weights in the exact order the 32x32x2 f32 MFMA consumes them; this
 * re-lays the Field's parameters into one flat buffer (done once per optimiser step).  The split-bf16
 * copies of the segments are written only when desc->mma_mode != RSN_MMA_F32: re-pack after changing it.
 * With RSN_MMA_F32_FOLDED (num_layers >= 2) the region of ONE of those copies -- the transposed x part of the last trunk layer,
 * which the exact-fp32 kernels never read -- holds the seed segment of the analytic-normal sweep instead: V[k][n] =
 * fl32(W_{L-1}[n][k] * w_density[n]) (one rounding), transposed like that copy, as three bf16 pieces hi + mid + lo = V (exact for
 * |V| >= 2^-110).  The folded training forward multiplies it by the ReLU bits of layer L-1; the RSN_MMA_F32
 * training forward forms the same pieces in registers, and its buffer is byte for byte what it was.  All sizes are unchanged.
 * RSN_MMA_F32_FOLDED also fills the split-bf16 copies of the OTHER segments the analytic-normal sweep reads -- the transposed x
 * parts of trunk layers 1 .. L-2 and the transposed encoded-input parts of layer 0 and of the skip layer -- in their own regions,
 * as the split-bf16 modes write them: the folded training forward runs those GEMMs on six of the nine products of the three pieces of
 * the weights and of the activations, the three smallest left out.  The remaining split-bf16 regions of the two exact-fp32 modes stay unwritten. */
size_t rsn_packed_weights_bytes(const rsn_field_desc* desc);
int rsn_pack_weights(const rsn_field_desc* desc, const rsn_field_params* params, float* packed,
                     size_t packed_bytes, void* stream);

/* The same result in ONE kernel launch per call (plus one for the split-bf16 copies and one for the bf16 ring stream
 * when desc->mma_mode asks for them) instead of one launch per segment: the per-segment job descriptors are kept in a
 * caller-owned device buffer `table` of rsn_pack_table_bytes() bytes.  They depend only on desc and on the parameter /
 * packed POINTERS: pass rebuild_table != 0 on the first call and whenever one of those changed (one asynchronous
 * host-to-device copy on `stream`), 0 otherwise (the optimiser step of a training loop: values change, pointers do
 * not). */
size_t rsn_pack_table_bytes(void);
int rsn_pack_weights_table(const rsn_field_desc* desc, const rsn_field_params* params, float* packed,
                           size_t packed_bytes, void* table, size_t table_bytes, int32_t rebuild_table, void* stream);

/* ---- samplers --------------------------------------------------------------------------------
 * rsn_sample_spaced replaces UniformSampler / ReciprocalSampler.generate_ray_samples
 * (reflect_sampling_nerf_model.py:148,292; reflect_sampling_nerf_components.py:14-36).
 * t_rand: [R,S+1] uniform [0,1) stratified jitter (training) or NULL (eval).
 * Outputs: spacing_bins [R,S+1] (normalised), euclid_bins [R,S+1] (ray parameter t). */
int rsn_sample_spaced(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, int32_t spacing, float tan,
                      const float* nears, const float* fars, const float* t_rand, float* spacing_bins,
                      float* euclid_bins, void* stream);

/* rsn_sample_pdf replaces PDFSampler.generate_ray_samples with include_original=False
 * (reflect_sampling_nerf_model.py:110,112,182,317).  weights [R,S_in], spacing_bins_in [R,S_in+1],
 * u_rand [R,S_out+1] or NULL.  S_in, S_out <= 1024. */
int rsn_sample_pdf(int32_t n_rays, const int32_t* n_dev, int32_t s_in, int32_t s_out, int32_t spacing, float tan,
                   float histogram_padding, const float* nears, const float* fars, const float* weights,
                   const float* spacing_bins_in, const float* u_rand, float* spacing_bins_out,
                   float* euclid_bins_out, void* stream);

/* ---- the field (dominant kernel) -------------------------------------------------------------
 * rsn_field_forward_frustum: for every sample of every ray: conical frustum -> Gaussian ->
 * contraction -> integrated positional encoding -> trunk MLP -> heads -> SH-34 -> mid MLP ->
 * colour.  Replaces get_blob + contract + get_density + get_pred_normals + get_reflection +
 * get_diff + get_tint + get_roughness + get_mid for one sampling level
 * (reflect_sampling_nerf_field.py:90-186; driven from reflect_sampling_nerf_model.py:151-175,
 * 185-209,293-310,319-336).  N = n_rays * n_samples; sample i of ray r is point r*S+i. */
int rsn_field_forward_frustum(const rsn_field_desc* desc, const float* packed, int32_t n_rays, const int32_t* n_dev,
                              int32_t n_samples, const float* origins, const float* directions,
                              const float* pixel_area, const float* euclid_bins, const rsn_field_outputs* out,
                              void* stream);

/* Training-mode variant of rsn_field_forward_frustum: identical outputs, plus the saved activations and
 * (when saved->normals != NULL) the analytic normals of Field.get_normals (reflect_sampling_nerf_field.py:
 * 125-127,134-135,146-147; reflect_sampling_nerf_model.py:159-160,194-195). */
int rsn_field_forward_frustum_train(const rsn_field_desc* desc, const float* packed, int32_t n_rays,
                                    const int32_t* n_dev, int32_t n_samples, const float* origins,
                                    const float* directions, const float* pixel_area, const float* euclid_bins,
                                    const rsn_field_outputs* out, const rsn_field_saved* saved, void* stream);

/* Several training-mode evaluations of the SAME field in ONE launch: the reflect branch of a step evaluates the field on
 * M reflected rays x S samples (model.py:292-297, 317-323) and on M points for get_inf_color (model.py:290) -- a few hundred
 * to ~1,250 tiles of 128 points on 256 persistent workgroups each.  Launched one by one every evaluation wastes its last
 * partial round of tiles and get_inf_color keeps 20 CUs busy for a whole launch; as jobs of one launch their tiles form
 * one tile space.  kind 0 = rsn_field_forward_frustum_train's arguments, kind 1 = rsn_field_forward_inf_train's. */
typedef struct rsn_field_job {
  int32_t kind;              /* 0: conical frustums of rays; 1: get_inf_color */
  int32_t n_rays;
  const int32_t* n_dev;      /* optional device-side ray count */
  int32_t n_samples;         /* kind 0 */
  const float* origins;      /* kind 0 */
  const float* directions;
  const float* pixel_area;   /* kind 0 */
  const float* euclid_bins;  /* kind 0 */
  const float* sqradius;     /* kind 1 */
  float* out_rgb;            /* kind 1: [n_rays,3] */
  const rsn_field_outputs* out;  /* kind 0 */
  const rsn_field_saved* saved;
} rsn_field_job;

int rsn_field_forward_train_jobs(const rsn_field_desc* desc, const float* packed, int32_t n_jobs,
                                 const rsn_field_job* jobs, void* stream);

/* ---- backward of one field level (training) ----------------------------------------------------
 * Upstream gradients per sample (NULL = zero) ... */
typedef struct rsn_field_grads_in {
  const float* sigma;        /* [N]   d loss / d sigma (from rsn_composite_backward)                 */
  const float* color;        /* [N,3] d loss / d colour                                              */
  const float* pred_normals; /* [N,3] d loss / d pred_normals (predicted-normal loss, model.py:403-404) */
  const float* n_dot_d;      /* [N]   d loss / d n_dot_d       (orientation loss, model.py:406-407)  */
  const float* roughness;    /* [N]   d loss / d sigmoid(roughness head) (rendered roughness, model.py:225-226) */
  /* fused normal losses: upstream gradients PER RAY of rsn_composite_io.pn_loss_ray / ori_loss_ray; the kernel forms
   * d/d pred_normals = ray_pn_loss[r] w (-2)(normals - pred_normals) and d/d n_dot_d = ray_ori_loss[r] w 2 max(0, n_dot_d)
   * itself from the level's weights, analytic normals (rsn_field_saved.normals) and forward outputs (pred_normals,
   * n_dot_d), so the per-sample gradient tensors never exist.  Added to pred_normals / n_dot_d above when both are given. */
  const float* ray_pn_loss;  /* [R] or NULL */
  const float* ray_ori_loss; /* [R] or NULL */
  const float* weights;      /* [N] compositing weights of the level (needed by the two above) */
} rsn_field_grads_in;

/* Pre-activation gradients of every linear layer, row-major, consumed by the weight-gradient GEMMs
 * dW = dY^T X (plain library GEMMs on the host) and by rsn_colsum (bias gradients). */
typedef struct rsn_field_grads_out {
  float* dz_rgb;    /* [N,4]   field_output_mid pre-sigmoid (3 live columns)                          */
  float* da_mid;    /* [N,128] mlp_mid pre-activation                      (bf16 under RSN_MMA_BF16)   */
  float* d_bott;    /* [N,W]   bottleneck output                           (bf16 under RSN_MMA_BF16;   *
                     *          RSN_MMA_F32_FOLDED: not touched, may be NULL)                           */
  float* dz_heads;  /* [N,16]  columns: 0 density, 1-3 normals, 4-6 diff, 8 roughness, 12-14 tint      */
  float* dy;        /* [L,N,W] pre-activation of trunk layer l             (bf16 under RSN_MMA_BF16)   */
  float* d_input;   /* [N]     d loss / d pixel_area (frustum) or d sqradius (inf); need_input_grad only */
} rsn_field_grads_out;

/* The backward sweeps of several evaluations of the same field in ONE launch (see rsn_field_job): kind 0 =
 * rsn_field_backward_frustum's arguments, kind 1 = rsn_field_backward_inf's (g_rgb = upstream gradient of its colour).
 * The sweeps of the two reflect levels and of get_inf_color are independent of each other once both levels' compositing
 * backward has produced the background gradient. */
typedef struct rsn_field_bwd_job {
  int32_t kind;
  int32_t n_rays;
  const int32_t* n_dev;
  int32_t n_samples;         /* kind 0 */
  int32_t need_input_grad;
  const float* origins;      /* kind 0 */
  const float* directions;
  const float* pixel_area;   /* kind 0 */
  const float* euclid_bins;  /* kind 0 */
  const float* sqradius;     /* kind 1 */
  const float* g_rgb;        /* kind 1: [n_rays,3] */
  const rsn_field_outputs* fwd;      /* kind 0 */
  const rsn_field_saved* saved;
  const rsn_field_grads_in* gin;     /* kind 0 */
  const rsn_field_grads_out* gout;
} rsn_field_bwd_job;

int rsn_field_backward_jobs(const rsn_field_desc* desc, const float* packed, int32_t n_jobs,
                            const rsn_field_bwd_job* jobs, void* stream);

/* rsn_field_backward_frustum: backward of rsn_field_forward_frustum_train.  fwd: the forward's per-sample
 * outputs (raw_density, diff, tint are read).  need_input_grad != 0 additionally carries the gradient through
 * the integrated positional encoding's variance back to pixel_area (reflected rays: pixel_area = pi*sqradius
 * depends on the non-detached rendered roughness, reflect_sampling_nerf_model.py:225-227,272,286). */
int rsn_field_backward_frustum(const rsn_field_desc* desc, const float* packed, int32_t n_rays, const int32_t* n_dev,
                               int32_t n_samples, const float* origins, const float* directions,
                               const float* pixel_area, const float* euclid_bins, const rsn_field_outputs* fwd,
                               const rsn_field_saved* saved, const rsn_field_grads_in* gin,
                               const rsn_field_grads_out* gout, int32_t need_input_grad, void* stream);

/* Training variant / backward of rsn_field_forward_inf (get_inf_color, field.py:190-201). */
int rsn_field_forward_inf_train(const rsn_field_desc* desc, const float* packed, int32_t n_rays, const int32_t* n_dev,
                                const float* directions, const float* sqradius, float* out_rgb,
                                const rsn_field_saved* saved, void* stream);
int rsn_field_backward_inf(const rsn_field_desc* desc, const float* packed, int32_t n_rays, const int32_t* n_dev,
                           const float* directions, const float* sqradius, const rsn_field_saved* saved,
                           const float* g_rgb, const rsn_field_grads_out* gout, int32_t need_input_grad,
                           void* stream);

/* rsn_field_forward_inf: get_inf_color (reflect_sampling_nerf_field.py:190-201): mean = 2d,
 * Sigma = 0.6*sqradius*(I - d d^T), no contraction, SH inputs zeroed; out_rgb [M,3]. */
int rsn_field_forward_inf(const rsn_field_desc* desc, const float* packed, int32_t n_rays, const int32_t* n_dev,
                          const float* directions, const float* sqradius, float* out_rgb, void* stream);

/* rsn_field_forward_gaussians: granular Field API (get_density(mean, cov) + heads,
 * reflect_sampling_nerf_field.py:122-186) on explicit, already contracted Gaussians:
 * means [N,3], cov_diag [N,3] (NULL => plain sin/cos encoding), view_dirs [N,3] (NULL => SH zeroed),
 * embedding [N,W] optional output (post-ReLU trunk output). */
int rsn_field_forward_gaussians(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                const float* means, const float* cov_diag, const float* view_dirs,
                                const rsn_field_outputs* out, float* embedding, void* stream);

/* rsn_field_forward_gaussians_train (ABI 16): the same evaluation in TRAINING mode -- reference field.py:122-137 with
 * requires_density_grad=True followed by get_normals() (field.py:146-147): the saved activations of the points
 * (rsn_field_saved, slab layout: rsn_train_saved_layout) and, in saved->normals [N,3], the analytic normals
 * -normalize(d raw_density / d mean) of the (contracted) means handed in.  Exact-fp32 fields (mma_mode RSN_MMA_F32) only:
 * the reduced / split precision training kernels take conical frustums, not Gaussians (RSN_ERR_UNSUPPORTED otherwise). */
int rsn_field_forward_gaussians_train(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                      const float* means, const float* cov_diag, const float* view_dirs,
                                      const rsn_field_outputs* out, float* embedding, const rsn_field_saved* saved,
                                      void* stream);

/* rsn_field_forward_embedding: the head getters of the granular Field API on a caller-supplied embedding [N,W]
 * (post-ReLU trunk output, as returned by get_density): get_pred_normals, get_diff, get_tint, get_roughness
 * (out->roughness = sigmoid, out->raw_density = density head), get_mid / get_low (out->color = diff + tint*mid
 * is NOT what get_mid returns: the mid colour itself is written to out->color when out->diff and out->tint are
 * NULL).  view_dirs NULL => SH inputs zeroed (get_low); roughness [N] NULL => softplus(roughness head)
 * (reflect_sampling_nerf_field.py:139-186). */
int rsn_field_forward_embedding(const rsn_field_desc* desc, const float* packed, int32_t n_points,
                                const float* embedding, const float* view_dirs, const float* roughness,
                                const rsn_field_outputs* out, void* stream);

/* ---- granular geometry (Field.get_blob / contract / get_reflection) --------------------------------------
 * rsn_gaussians: conical frustum -> Gaussian per sample (reflect_sampling_nerf_field.py:90-96 ->
 * Frustums.get_gaussian_blob): per-sample origins/directions [N,3], pixel_area/starts/ends [N] ->
 * mean [N,3], cov [N,3,3]. */
int rsn_gaussians(int64_t n, const float* origins, const float* directions, const float* pixel_area,
                  const float* starts, const float* ends, float* mean, float* cov, void* stream);
/* rsn_contract: reflect_sampling_nerf_field.py:98-119: mean' and J cov J with the diagonal clamped >= 0. */
int rsn_contract(int64_t n, const float* mean, const float* cov, float* mean_out, float* cov_out, void* stream);
/* rsn_reflection: reflect_sampling_nerf_field.py:203-207: n_dot_d [N] and normalize(d - 2 (n.d) n) [N,3]. */
int rsn_reflection(int64_t n, const float* directions, const float* normals, float* reflections, float* n_dot_d,
                   void* stream);

/* ---- compositing ------------------------------------------------------------------------------
 * rsn_composite: RaySamples.get_weights + RGB/Accumulation/Depth(median)/Normals/Semantic
 * renderers for one level (reflect_sampling_nerf_model.py:154-156,176-177,188-190,210-227,
 * 296-297,311,322-323,337,341).  One wavefront per ray, wave-level scan for the transmittance.
 * background: 0 = none ("random"), 1 = white, 2 = per-ray tensor bg_rgb [R,3].
 * flags: RSN_COMP_EVAL = RGBRenderer in eval mode (nan_to_num the colours, clamp composites to [0,1]);
 *        RSN_COMP_CLIP_RGB = additionally apply the model's own torch.clip(rgb, 0, 1)
 *        (reflect_sampling_nerf_model.py:177,211; not applied to the reflect composites, :311,337).
 * Outputs (NULL = skip): weights [R,S], rgb [R,3], accumulation
 * [R], depth [R]; surface attributes from the optional per-sample inputs: diff_out [R,3] (white
 * background), tint_out [R,3] (no background), normals_out [R,3] (normalised, eps 1e-10),
 * roughness_out [R]. */
typedef struct rsn_composite_io {
  const float* sigma;        /* [R,S] */
  const float* euclid_bins;  /* [R,S+1] */
  const float* color;        /* [R,S,3] */
  const float* bg_rgb;       /* [R,3] or NULL */
  const float* diff;         /* [R,S,3] or NULL */
  const float* tint;         /* [R,S,3] or NULL */
  const float* pred_normals; /* [R,S,3] or NULL */
  const float* roughness;    /* [R,S] or NULL */
  float* weights;
  float* rgb;
  float* accumulation;
  float* depth;
  float* diff_out;
  float* tint_out;
  float* normals_out;
  float* roughness_out;
  /* training: the per-sample loss terms of get_loss_dict (reflect_sampling_nerf_model.py:395-407) reduced per ray in the
   * compositing epilogue, where the weights are in registers:
   *   pn_loss_ray[r]  = sum_s w |normals - pred_normals|^2      (predicted_normal_loss_*: the sum over r)
   *   ori_loss_ray[r] = sum_s w max(0, n_dot_d)^2               (orientation_loss_*)
   * normals = the analytic normals of the training forward (rsn_field_saved.normals); all NULL = skip. */
  const float* normals;      /* [R,S,3] or NULL */
  const float* n_dot_d;      /* [R,S] or NULL */
  float* pn_loss_ray;        /* [R] or NULL (needs normals and pred_normals) */
  float* ori_loss_ray;       /* [R] or NULL (needs n_dot_d) */
} rsn_composite_io;

#define RSN_COMP_EVAL 1
#define RSN_COMP_CLIP_RGB 2
int rsn_composite(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, int32_t background, int32_t flags,
                  const rsn_composite_io* io, void* stream);

/* rsn_composite_backward: backward of rsn_composite in training mode (no eval clamp).
 * g_rgb [R,3]: gradient w.r.t. the rgb output (after the model's clip when RSN_COMP_CLIP_RGB: masked where the
 * unclipped composite left [0,1]); g_roughness [R] (or NULL): gradient w.r.t. the rendered roughness;
 * weights: the forward's weights [R,S].  detach_weights != 0: the weights were detached (reflect levels,
 * model.py:297,323): no gradient reaches sigma.  Outputs (NULL = skip): g_sigma [R,S], g_color [R,S,3],
 * g_roughness_sample [R,S], g_bg [R,3] (background == 2). */
typedef struct rsn_composite_bwd_io {
  const float* sigma;
  const float* euclid_bins;
  const float* color;
  const float* bg_rgb;
  const float* roughness;       /* [R,S] per-sample sigmoid roughness (or NULL) */
  const float* weights;
  const float* g_rgb;
  const float* g_roughness;
  const float* g_accumulation;  /* [R] or NULL: gradient w.r.t. sum_s w (model.py:240-241: white*(1-acc_fine)) */
  float* g_sigma;
  float* g_color;
  float* g_roughness_sample;
  float* g_bg;
} rsn_composite_bwd_io;

int rsn_composite_backward(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, int32_t background, int32_t flags,
                           int32_t detach_weights, const rsn_composite_bwd_io* io, void* stream);

/* Distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15; nerfstudio's lossfun_distortion) of one level's compositing
 * weights, an opt-in regulariser of the training step.  Per ray, with the S intervals of the samplers' normalised spacing bins
 * s_0 <= ... <= s_S (spacing_bins [R,S+1], ascending), midpoints m_i = (s_i + s_{i+1}) / 2, widths d_i = s_{i+1} - s_i and the
 * weights w_i of rsn_composite (weights [R,S]):
 *   L_ray        = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 *   dL_ray/dw_k  = 2 sum_j w_j |m_k - m_j| + (2/3) w_k d_k
 * The double sum is evaluated in O(S) from prefix sums of w and w m along the sorted ray,
 *   sum_j w_j |m_k - m_j| = m_k (W_<k - W_>k) - (WM_<k - WM_>k),
 * which subtracts numbers of order 1 for a result that is tiny on a compact ray: midpoints, widths, prefixes and the per-ray sum are
 * fp64 (exact from the fp32 bits up to the scans' roundings) and the result is rounded to fp32 once.
 * One wave per ray, 64-sample chunks with carried scans, no atomics, a fixed order of addition: the same inputs give the same bits.
 * n_dev (or NULL): device-side ray count, min(n_rays, *n_dev) rows are processed and the rows behind are not touched.
 *
 * rsn_distortion_forward: loss_ray [R] = L_ray, unscaled.
 * rsn_distortion_backward: g_w[k] = g_loss_ray[r] dL_ray/dw_k is recomputed (nothing [R,S]-sized is kept from the forward) and
 *   carried to sigma through the transmittance by rsn_composite_backward's rule,
 *     g_sigma[k] = delta_k (g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i),  delta_k from euclid_bins [R,S+1], T_{k+1} = exp(-sum_{j<=k} delta_j sigma_j),
 *   sigma [R,S] and euclid_bins being the inputs of the rsn_composite call whose weights the forward read.  It takes no weights: it
 *   re-derives them in fp64, w_k = (1 - exp(-delta_k sigma_k)) T_k.  rsn_composite's fp32 weights are good to 2^-24 of T_k, not of
 *   w_k, and both g_w and the suffix sum are proportional to single weights; from them a thin sample's gradient is off by thousands
 *   of fp32 roundings.  The suffix sum is added up from the far end of the ray, not taken as total - prefix.
 *   accumulate != 0: the value, rounded to fp32, is ADDED to g_sigma [R,S] (the training step adds it to what
 *   rsn_composite_backward wrote); 0: it overwrites.  n_samples <= 4096 (RSN_ERR_UNSUPPORTED above).
 *
 * RSN_ERR_INVALID_ARGUMENT before any launch: n_rays < 0, n_samples < 1, or, with n_rays > 0, a NULL pointer other than n_dev.
 * n_rays == 0 launches nothing. */
int rsn_distortion_forward(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* spacing_bins, const float* weights,
                           float* loss_ray, void* stream);
int rsn_distortion_backward(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* spacing_bins,
                            const float* euclid_bins, const float* sigma, const float* g_loss_ray, float* g_sigma,
                            int32_t accumulate, void* stream);

/* Standalone encoders: what calling the Field's encoding modules directly computes.
 * rsn_sh34_encode: IntegratedSHEncoding.forward (components.py:52-140): 34 real-SH terms of bands l = 1, 2, 4, 8 of
 *   `directions` [n,3], band l attenuated by exp(-l(l+1)/2 * roughness) (roughness [n] or NULL = 0); out [n,34].
 * rsn_ipe_encode: nerfstudio NeRFEncoding(3, 16, 0, 16, include_input=True).forward(means, covs) as the Field calls
 *   it (field.py:129-131): out [n,99] = [sin block 48 | sin(.+pi/2) block 48 | raw 3], each block coord-major /
 *   freq-minor, scaled by exp(-0.5 var f^2) when cov_diag [n,3] is given.  freqs16: HOST array of the 16 frequencies. */
int rsn_sh34_encode(int64_t n, const float* directions, const float* roughness, float* out, void* stream);
int rsn_ipe_encode(int64_t n, const float* means, const float* cov_diag, const float* freqs16, float* out,
                   void* stream);

/* rsn_weight_grad: dW[n][col_map ? col_map[k] : k] += sum_m dY[m][n] * X[m][k]  and  db[n] += sum_m dY[m][n]
 * (n < n_out <= 256, k < k_in <= 256; entries with col_map[k] < 0 are dropped).  The weight-gradient GEMM of
 * every linear layer of the Field: a reduction over all N sample points with the output tile stationary in MFMA
 * accumulators.  dW / db are ACCUMULATED (the caller zeroes them once per step); row-major, leading dims in floats. */
int rsn_weight_grad(int64_t n_points, const float* dy, int32_t ld_dy, int32_t n_out, const float* x, int32_t ld_x,
                    int32_t k_in, const int32_t* col_map, float* dw, int32_t ld_dw, float* db, void* stream);

/* rsn_weight_grad_multi: the same reduction over n_segments (<= 8) point sets in ONE launch -- segment s holds
 * n_points[s] rows of dy[s] / x[s] (HOST arrays of device pointers; common leading dimensions).  The five field
 * evaluations of one training step (model.py:146-292) share their weights, so the per-launch cost (the atomic flush
 * of the stationary output tile) is paid once per layer instead of once per layer and evaluation. */
int rsn_weight_grad_multi(int32_t n_segments, const int64_t* n_points, const float* const* dy, int32_t ld_dy,
                          int32_t n_out, const float* const* x, int32_t ld_x, int32_t k_in, const int32_t* col_map,
                          float* dw, int32_t ld_dw, float* db, void* stream);

/* The same reduction in the Field's MMA mode (rsn_field_desc.mma_mode), over the same fp32 buffers:
 *   RSN_MMA_F32 / RSN_MMA_BF16X3  the exact kernel above;
 *   RSN_MMA_BF16X6  both operands split exactly into bf16 triples inside the kernel, 6 products on
 *                   v_mfma_f32_32x32x16_bf16 with fp32 accumulation: fp32-equivalent (dropped terms <= 2^-24 relative);
 *   RSN_MMA_BF16    operands rounded to bf16 (the opt-in reduced-precision training mode), fp32 accumulation.
 * Bias sums are exact fp32 in every mode.  Shapes / alignments the vector-load layout does not cover take the exact
 * kernel. */
int rsn_weight_grad_multi_mode(int32_t n_segments, const int64_t* n_points, const float* const* dy, int32_t ld_dy,
                               int32_t n_out, const float* const* x, int32_t ld_x, int32_t k_in, const int32_t* col_map,
                               float* dw, int32_t ld_dw, float* db, int32_t mma_mode, void* stream);

/* The same with DEVICE-side segment lengths: segment s holds min(n_points_max[s], *n_dev[s] * per_count[s]) rows when
 * n_dev[s] is not NULL (HOST array of device pointers to int32 counts; per_count = rows per counted unit, i.e. samples
 * per ray), n_points_max[s] rows otherwise.  The reflect branch of a training step runs on the M rays behind the mask
 * (reference model.py:229,259-290); M is produced on the device by rsn_reflect_setup and never read by the host, so the
 * step has no device-to-host synchronisation.  The grid is sized for the upper bounds.
 * operand_bf16 (RSN_MMA_BF16 only): bit 0 = the x rows, bit 1 = the dy rows ARE bf16 in memory (the reduced-precision
 * training mode keeps its wide buffers as bf16, see rsn_field_saved / rsn_field_grads_out); leading dimensions count
 * elements.  bf16 dy rows need n_out > 32; a shape the vector-load layout does not cover is an error, not a fallback. */
int rsn_weight_grad_multi_dev(int32_t n_segments, const int64_t* n_points_max, const int32_t* const* n_dev,
                              const int32_t* per_count, const float* const* dy, int32_t ld_dy, int32_t n_out,
                              const float* const* x, int32_t ld_x, int32_t k_in, const int32_t* col_map, float* dw,
                              int32_t ld_dw, float* db, int32_t mma_mode, int32_t operand_bf16, void* stream);

/* Several weight-gradient reductions of ONE shape over the SAME segments in one launch (the trunk layers of a training step:
 * 256 x 256 each, reference autograd of reflect_sampling_nerf_field.py:54-60's MLP).  The workgroups are dealt to the jobs
 * round-robin; every workgroup still flushes one output tile, so n_jobs layers pay ONE atomic-flush phase and one launch
 * ramp.  dy[s] / x[s]: the job's rows of segment s (HOST arrays of n_segments device pointers); other arguments as
 * rsn_weight_grad_multi_dev. */
typedef struct rsn_wgrad_job {
  const float* const* dy;  /* [n_segments] -> [n_s, ld_dy]                        */
  const float* const* x;   /* [n_segments] -> [n_s, ld_x]                         */
  const int32_t* col_map;  /* optional: packed column k -> destination column / -1 */
  float* dw;               /* [n_out, ld_dw], accumulated                          */
  int32_t ld_dw;
  float* db;               /* [n_out] or NULL, accumulated                         */
} rsn_wgrad_job;
int rsn_weight_grad_jobs(int32_t n_segments, const int64_t* n_points_max, const int32_t* const* n_dev,
                         const int32_t* per_count, int32_t n_jobs, const rsn_wgrad_job* jobs, int32_t ld_dy, int32_t n_out,
                         int32_t ld_x, int32_t k_in, int32_t mma_mode, int32_t operand_bf16, void* stream);

/* ORDERED weight-gradient reduction (ABI 18): the same sums as rsn_weight_grad_multi_dev / rsn_weight_grad_jobs with a fixed order of
 * addition, for bit-reproducible training.  The calls above add every wave's partial tile to dW / db with fp32 atomics, whose order of
 * arrival differs from run to run (the last bits of the gradients differ); here every wave stores its partial tile to a slot of
 * `workspace`, and a second kernel on the same stream sums the slots of each output element in ascending slot order and adds the sum
 * to dW / db with one plain read-modify-write.  No atomics.
 * Guarantee: the same library build, the same device, the same arguments (sizes, leading dimensions, mode, alignment of the pointers)
 * and the same operand bits -- the device-side counts included -- give the same output bits, in the same process or another one.
 * It does NOT hold across devices with different CU counts (the grid, and with it the partition of the points, follows the CU count)
 * or across library builds.  Accumulation into non-zero dW / db, ld_dw, col_map (-1 entries) and rows >= n_out behave as in the
 * atomic calls; the result differs from theirs by the order of the additions only.
 * Workspace rule: `workspace` is device memory of at least rsn_weight_grad_workspace_bytes(...) bytes for the same segment upper
 * bounds, n_jobs (1 for rsn_weight_grad_multi_dev_ordered), shape, mode and operand_bf16, 16-byte aligned; a smaller one is
 * RSN_ERR_INVALID_ARGUMENT before any launch, with the needed size in rsn_last_error().  Its contents on entry do not matter and are
 * undefined on return; launches on ONE stream may share it (the library neither allocates nor synchronises).  The size is an upper
 * bound computed on the host without reading the device counts: 4 slots per workgroup (at most one workgroup per CU) of 192 + 2048 * NKB
 * floats, NKB = 2 / 4 / 8 for k_in <= 64 / 128 / 256 -- 68 MB for a 256-column output on 256 CUs.  rsn_weight_grad_workspace_bytes returns 0 (and sets rsn_last_error) on bad arguments. */
size_t rsn_weight_grad_workspace_bytes(int32_t n_segments, const int64_t* n_points_max, int32_t n_jobs, int32_t n_out, int32_t k_in,
                                       int32_t mma_mode, int32_t operand_bf16);
int rsn_weight_grad_multi_dev_ordered(int32_t n_segments, const int64_t* n_points_max, const int32_t* const* n_dev,
                                      const int32_t* per_count, const float* const* dy, int32_t ld_dy, int32_t n_out,
                                      const float* const* x, int32_t ld_x, int32_t k_in, const int32_t* col_map, float* dw,
                                      int32_t ld_dw, float* db, int32_t mma_mode, int32_t operand_bf16, void* workspace,
                                      size_t workspace_bytes, void* stream);
int rsn_weight_grad_jobs_ordered(int32_t n_segments, const int64_t* n_points_max, const int32_t* const* n_dev,
                                 const int32_t* per_count, int32_t n_jobs, const rsn_wgrad_job* jobs, int32_t ld_dy, int32_t n_out,
                                 int32_t ld_x, int32_t k_in, int32_t mma_mode, int32_t operand_bf16, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Parameter gradients of field_output_bottleneck and of the x part of mlp_mid.layers.0 from the reductions of the FOLDED training
 * step (RSN_MMA_F32_FOLDED), with W_mx = mid_w[:, 34:34+width] (row stride ld_mid) and n_mid = the rows of mlp_mid.layers.0:
 *   c [n_mid, width] (row stride ld_c) = sum over points of d a_mid (x) act[L-1]      s [n_mid] = sum over points of d a_mid
 *   d_bott_w [width, width] += W_mx^T c         d_bott_b [width] += W_mx^T s         d_mid_w[:, 34:34+width] += c W_b^T + s (x) b_b
 * (d_mid_w: the gradient tensor of mlp_mid.layers.0.weight, row stride ld_mid; bott_w [width, width], bott_b [width]).  `width` is the
 * width of the PARAMETER tensors.  fp64 accumulation in ascending index order, one thread per output element, one fp32 rounding of
 * the sum and one fp32 add into the gradient: the same inputs give the same bits.  Linear in (c, s): one call per reduction. */
int rsn_unfold_bottleneck_grads(int32_t width, int32_t n_mid, const float* c, int32_t ld_c, const float* s, const float* mid_w,
                                int32_t ld_mid, const float* bott_w, const float* bott_b, float* d_bott_w, float* d_bott_b,
                                float* d_mid_w, void* stream);

/* get_loss_dict on per-ray quantities only (training step: the per-sample normal terms arrive reduced per ray from
 * rsn_composite): losses8[k] = the UNSCALED terms (0-3 MSE means of rgb4[k] against image; 4,5 = sum_r pn_loss_ray2[lv][r];
 * 6,7 = sum_r ori_loss_ray2[lv][r]); g_rgb4[k] = coef8[k] * d term / d rgb4[k]. */
int rsn_loss_rays_forward(int32_t n_rays, const float* image, const float* const* rgb4, const float* const* pn_loss_ray2,
                          const float* const* ori_loss_ray2, const float* coef8, float* losses8, float* const* g_rgb4,
                          void* stream);

/* its chain rule: g_rgb4[k] *= upstream8[k] in place; g_pn_ray2[lv][r] = coef8[4+lv] * upstream8[4+lv],
 * g_ori_ray2[lv][r] = coef8[6+lv] * upstream8[6+lv] (upstream8: DEVICE pointer). */
int rsn_loss_rays_backward(int32_t n_rays, const float* upstream8, const float* coef8, float* const* g_rgb4,
                           float* const* g_pn_ray2, float* const* g_ori_ray2, void* stream);

/* rsn_colsum: out[c] (+)= sum_r x[r*ld + c], c < n_cols (bias gradients = column sums of dY). */
int rsn_colsum(int64_t n_rows, int32_t n_cols, int32_t ld, const float* x, float* out, int32_t accumulate,
               void* stream);

/* rsn_ray_sum: out[r] = sum_s x[r*S + s]  (per-ray total of a per-sample quantity). */
int rsn_ray_sum(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* x, float* out, void* stream);

/* rsn_reflect_backward: gradient of the secondary-ray construction w.r.t. the rendered roughness
 * (reflect_sampling_nerf_model.py:272,286): sqradius = 2|n.d| roughness^2, pixel_area = pi * sqradius.
 * g_roughness[ray_index[i]] = (g_sqradius[i] + pi * g_pixel_area[i]) * 2|n.d| * 2 roughness, zero elsewhere. */
int rsn_reflect_backward(int32_t n_rays, const int32_t* n_masked, const int32_t* ray_index, const float* n_dot_d,
                         const float* roughness, const float* g_sqradius, const float* g_pixel_area,
                         float* g_roughness, void* stream);

/* rsn_reflect_default_backward: rays that are NOT reflected keep mid_reflect_{coarse,fine} = white*(1-acc_fine)
 * with a live accumulation (reflect_sampling_nerf_model.py:240-241):
 * g_accumulation[r] = mask[r] ? 0 : -sum_c (g_reflect_coarse[r,c] + g_reflect_fine[r,c]). */
int rsn_reflect_default_backward(int32_t n_rays, const uint8_t* mask, const float* g_reflect_coarse,
                                 const float* g_reflect_fine, float* g_accumulation, void* stream);

/* ---- reflection rays --------------------------------------------------------------------------
 * rsn_reflect_setup: reflect_sampling_nerf_model.py:222-229,240-241,267-289: n_dot_d, mask =
 * (acc > 1e-2) & (n_dot_d < 0), stable compaction of the masked rays, secondary-ray origins /
 * directions / sqradius / pixel_area / nears / fars, and the default reflect colour
 * white*(1-acc) for every ray.  Outputs: mask [R] (uint8), n_masked (device int32), ray_index [R]
 * (first M entries = original ray of compacted ray i), compacted [M,*] arrays, reflect_default [R,3]
 * written to BOTH reflect_coarse and reflect_fine. */
typedef struct rsn_reflect_io {
  const float* origins;       /* [R,3] */
  const float* directions;    /* [R,3] */
  const float* accumulation;  /* [R]   accumulation_fine */
  const float* depth;         /* [R]   depth_fine (median) */
  const float* pred_normals;  /* [R,3] rendered, normalised */
  const float* roughness;     /* [R]   rendered */
  uint8_t* mask;              /* [R] */
  int32_t* n_masked;          /* [1] */
  int32_t* ray_index;         /* [R] */
  float* n_dot_d;             /* [R] */
  float* origins2;            /* [R,3] (first M valid) */
  float* directions2;         /* [R,3] */
  float* sqradius;            /* [R]   */
  float* pixel_area2;         /* [R]   pi * sqradius */
  float* nears2;              /* [R]   0 */
  float* fars2;               /* [R]   reflect_far */
  float* reflect_coarse;      /* [R,3] white*(1-acc) */
  float* reflect_fine;        /* [R,3] white*(1-acc) */
  int32_t* workspace;         /* rsn_reflect_workspace_bytes(R) bytes, contents irrelevant (per-block counts) */
} rsn_reflect_io;

size_t rsn_reflect_workspace_bytes(int32_t n_rays);
int rsn_reflect_setup(int32_t n_rays, float reflect_far, const rsn_reflect_io* io, void* stream);

/* rsn_reflect_combine: out[ray_index[i]] = clip(diff[ray_index[i]] + tint[ray_index[i]] * comp[i], 0, 1)
 * for i < *n_masked (reflect_sampling_nerf_model.py:312-313,338-339). */
int rsn_reflect_combine(int32_t n_rays_max, const int32_t* n_masked, const int32_t* ray_index, const float* diff,
                        const float* tint, const float* comp, float* out, void* stream);

/* rsn_reflect_combine_backward: backward of rsn_reflect_combine w.r.t. the composite (diff/tint are detached,
 * reflect_sampling_nerf_model.py:216,218): g_comp[i] = g_out[r] * tint[r] where 0 <= diff[r]+tint[r]*comp[i] <= 1. */
int rsn_reflect_combine_backward(int32_t n_rays_max, const int32_t* n_masked, const int32_t* ray_index,
                                 const float* diff, const float* tint, const float* comp, const float* g_out,
                                 float* g_comp, void* stream);

/* ---- the two steps after the hot path in a training iteration ------------------------
 * rsn_loss_forward_backward: get_loss_dict (reflect_sampling_nerf_model.py:346-430).  Term order of losses8 /
 * coef8: loss_mid_coarse, loss_mid_fine, loss_reflect_mid_coarse, loss_reflect_mid_fine (MSE means against `image`
 * [R,3]), predicted_normal_loss_{coarse,fine} = sum w |normals - pred_normals|^2, orientation_loss_{coarse,fine} =
 * sum w max(0, n_dot_d)^2.  losses8 (device, overwritten) receives the UNSCALED terms; the gradient outputs
 * (w.r.t. rgb4, pred_normals2, n_dot_d2; all other inputs are constants of the loss) are scaled by coef8
 * (host array, the model's loss_coefficients incl. the 50-step warm-up of reflect_sampling_nerf_pipeline.py:79-91).
 * The *4 / *2 arguments are HOST arrays of device pointers (coarse, fine order).
 * losses8 is bit-reproducible: the blocks' partial sums go to a buffer the library owns (one per device) and are added in
 * fp64 in a fixed order by a second launch, so two calls on different streams of one device must not overlap. */
int rsn_loss_forward_backward(int32_t n_rays, int32_t s_coarse, int32_t s_fine, const float* image,
                              const float* const* rgb4, const float* const* weights2, const float* const* normals2,
                              const float* const* pred_normals2, const float* const* n_dot_d2, const float* coef8,
                              float* losses8, float* const* g_rgb4, float* const* g_pred_normals2,
                              float* const* g_n_dot_d2, void* stream);

/* Chain rule for the gradients rsn_loss_forward_backward wrote: g_rgb4[k] *= upstream8[k], g_pred_normals2[lv] *=
 * upstream8[4 + lv], g_n_dot_d2[lv] *= upstream8[6 + lv], in place, upstream8 = d total / d (scaled loss k) in DEVICE
 * memory (what autograd hands to the backward of get_loss_dict's terms; all ones for loss = sum of the terms). */
int rsn_loss_scale_grads(int32_t n_rays, int32_t s_coarse, int32_t s_fine, const float* upstream8, float* const* g_rgb4,
                         float* const* g_pred_normals2, float* const* g_n_dot_d2, void* stream);

/* rsn_radam_step: one RAdam update (torch.optim.RAdam semantics; the reference's optimiser for the "fields" group,
 * reflect_sampling_nerf_config.py:50-53: lr 1e-3, eps 1e-15, betas 0.9/0.999) over all parameter tensors in one
 * launch.  HOST arrays of device pointers; grads[t] == NULL skips tensor t (unused parameter); step counts from 1. */
int rsn_radam_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int32_t* sizes, int32_t step, float lr, float beta1, float beta2,
                   float eps, void* stream);

/* ---- guarded optimiser step (additive to ABI 18; opt-in, rsn_radam_step itself is unchanged): clipping of the global
 * gradient norm (nerfstudio OptimizerConfig.max_norm -> torch.nn.utils.clip_grad_norm_) and the skip of an iteration whose
 * gradients hold an inf or a NaN (what torch's GradScaler.step does under the reference's mixed_precision=True).  Two
 * launches, no atomics, no hand-off between workgroups inside a launch, no host read.
 *
 * rsn_grad_sumsq: for every tensor t with grads[t] != NULL, fp64 partial sums of squares at fixed positions of `workspace`
 * (rsn_grad_sumsq_workspace_bytes; 8-byte aligned; it needs no zeroing: every position the next call reads is written by
 * every call).  Each fp32 element is converted to fp64 and squared there, which is exact.  Tensor t is cut into quads of 4
 * consecutive elements; with B <= 8 blocks of 256 threads per tensor (B = ceil(max size / 1024), a function of `sizes`
 * alone), thread k of the 256 B threads adds the squares of quads k, k + 256 B, ... element by element, threads
 * 0 .. size % 4 - 1 then one element of the tail each; a block sums its threads by a wave butterfly and its four wave sums
 * in index order and stores the result in slot (t, block).  16-byte aligned tensors are read as 16-byte vectors, any other
 * element by element: the same sums in the same order.  At most 48 tensors, sizes >= 0. */
size_t rsn_grad_sumsq_workspace_bytes(int32_t n_tensors, const int32_t* sizes);  /* 0 + rsn_last_error on bad arguments */
int rsn_grad_sumsq(int32_t n_tensors, const float* const* grads, const int32_t* sizes, void* workspace,
                   size_t workspace_bytes, void* stream);

#define RSN_GUARD_MAX_TENSORS 48
/* Written by rsn_radam_step_guarded on every call, in DEVICE memory (8-byte aligned), zero-filled by the caller before the
 * first call.  Entries of tensors beyond n_tensors or without a gradient are 0. */
typedef struct rsn_guard_stats {
  float last_norm;            /* (float)sqrt(total_sq) of this call */
  float last_coef;            /* the factor the gradients were read with (1 without clipping) */
  int32_t last_skipped;       /* 1: this call changed no parameter and no moment */
  int32_t skipped_total;      /* its own previous value, plus one on a skip */
  int32_t last_skipped_step;  /* `step` of the last skipped call; 0: none so far */
  int32_t reserved;
  double per_tensor_sq[RSN_GUARD_MAX_TENSORS];               /* sum of squares per tensor, this call */
  double per_tensor_sq_at_last_skip[RSN_GUARD_MAX_TENSORS];  /* the same of the last skipped call: which one blew up */
} rsn_guard_stats;

/* rsn_radam_step_guarded: rsn_radam_step's arguments and update, preceded in every workgroup by the sum of the partials
 * that rsn_grad_sumsq left in `workspace` for the same (n_tensors, grads, sizes), in a fixed order and in fp64: per tensor
 * over its slots, then over the tensors in index order (total_sq).  With norm = (float)sqrt(total_sq):
 *   - skip_nonfinite != 0 and total_sq not finite: no parameter and no moment is written;
 *   - else coef = min(1.0f, max_norm / (norm + 1e-6f)) in fp32, torch.nn.utils.clip_grad_norm_'s formula (a NaN stays a
 *     NaN, as torch's clamp keeps it); max_norm <= 0 or +inf: no clipping, coef = 1.  The update is rsn_radam_step's on
 *     grads[t][i] * coef; with coef = 1 it has rsn_radam_step's bits.  Without skip_nonfinite a non-finite norm simply
 *     goes through this arithmetic (torch: error_if_nonfinite=False).
 * grads themselves are NOT rewritten (torch scales .grad in place; nothing in this library reads it after the step).
 * One workgroup writes *stats.
 * A skipped call leaves the step counting to the caller, who passes `step` and the learning rate: the Python optimiser
 * advances both on every call, skipped or not, so a skip costs one step of bias correction against torch's GradScaler,
 * which does not advance a skipped step -- and in exchange there is no device-side counter, no host read and no optimiser
 * state beyond RAdam's. */
int rsn_radam_step_guarded(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const int32_t* sizes, int32_t step, float lr, float beta1,
                           float beta2, float eps, float max_norm, int32_t skip_nonfinite, const void* workspace,
                           size_t workspace_bytes, rsn_guard_stats* stats, void* stream);


/* ---- standalone data path (ABI 17): training batches and rendered views from a device-resident posed image set, and the
 * SSIM metric (reference reflect_sampling_nerf_datamanager.py:49-58 next_train, reflect_sampling_nerf_model.py:468-479).
 *
 * Rays: nerfstudio 0.3 Cameras._generate_rays_from_coords, perspective camera.  For pixel (y, x) of a camera with pose
 * c2w [3,4] (row-major) and intrinsics fx, fy, cx, cy: camera-space direction v = ((x+.5-cx)/fx, -(y+.5-cy)/fy, -1);
 * directions = normalize(c2w[:, :3] v); origins = c2w[:, 3]; pixel_area = |d - d_x1| * |d - d_y1| with d_x1 / d_y1 the
 * directions of the x+1 / y+1 neighbours formed the same way (the differences are evaluated in a cancellation-free
 * rearrangement, so pixel_area is accurate to fp32 rounding rather than to the ~1/f-amplified error of the literal
 * subtraction).  Both kernels below run the same device function: equal (i, y, x) give bit-identical rays. */

/* rsn_sample_camera_rays: one training batch of n_rays rays, uniform over all N*H*W pixels with replacement (nerfstudio's
 * PixelSampler).  images: uint8 [N,H,W,4] RGBA (alpha 255 for RGB sources), c2w: fp32 [N,3,4]; N*H*W < 2^32.
 * Pixel of ray r (bit-exact recipe):
 *   (u, -, -, -) = Philox4x32-10(counter = (step, r, 0, 0), key = (seed, rank))   (Random123's philox4x32, 10 rounds)
 *   flat = (uint32)(((uint64)u * (N*H*W)) >> 32);  i = flat / (H*W);  y = (flat % (H*W)) / W;  x = flat % W
 * Outputs: origins / directions / rgb [R,3], pixel_area [R,1], indices int32 [R,3] = (i, y, x) (nerfstudio's
 * batch["indices"]); rgb = c/255 * a/255 + (1 - a/255) per channel in fp32 (white background, as get_loss_dict blends). */
int rsn_sample_camera_rays(int32_t n_images, int32_t height, int32_t width, const uint8_t* images, const float* c2w,
                           float fx, float fy, float cx, float cy, int32_t n_rays, uint32_t seed, uint32_t rank,
                           uint32_t step, float* origins, float* directions, float* pixel_area, float* rgb,
                           int32_t* indices, void* stream);

/* rsn_camera_rays_image: the rays of every pixel of ONE camera (c2w: [3,4]), row-major [H*W]: origins / directions
 * [H*W,3], pixel_area [H*W,1]. */
int rsn_camera_rays_image(int32_t height, int32_t width, const float* c2w, float fx, float fy, float cx, float cy,
                          float* origins, float* directions, float* pixel_area, void* stream);

/* rsn_ssim: torchmetrics structural_similarity_index_measure(pred, target) with the defaults the reference uses
 * (model.py:131,470) of two fp32 [H,W,3] images (H, W >= 11), written to out[0] (device).  11-tap Gaussian, sigma 1.5
 * (taps exp(-k^2/(2 sigma^2)), k = -5..5, normalised; 2-D window = their outer product); L = *data_range (device: the
 * caller's max(max(pred)-min(pred), max(target)-min(target))); C1 = (0.01 L)^2, C2 = (0.03 L)^2; per window the means,
 * variances E[x^2]-mu^2 and covariance; the SSIM map averaged over the 3 channels and the (H-10) x (W-10) positions whose
 * window lies inside the image (torchmetrics' reflect-pad-then-crop-by-5 keeps exactly those).  Per-workgroup partial
 * sums in `workspace` (rsn_ssim_workspace_bytes, 8-byte aligned) are added in a fixed order: bit-reproducible. */
size_t rsn_ssim_workspace_bytes(int32_t height, int32_t width);
int rsn_ssim(int32_t height, int32_t width, const float* pred, const float* target, const float* data_range,
             void* workspace, size_t workspace_bytes, float* out, void* stream);


/* ---- image pyramids (additive to ABI 18: no existing call changes): every image of the set at 1, 1/2, 1/4, ... of its size, and
 * training batches drawn across the scales (mip-NeRF's multi-scale protocol, Barron et al. 2021).
 *
 * Level l = 0 .. L-1 of an H x W image has (H >> l) x (W >> l) pixels; 1 <= L <= RSN_PYRAMID_MAX_LEVELS, and H and W must be
 * divisible by 2^(L-1).  Level 0 is the uint8 RGBA image set itself (images [N,H,W,4]); it is never copied.  The levels l >= 1 are
 * white-blended fp32 [*, 3] in ONE allocation `pyramid`, level after level and within a level image after image, row-major.
 * Offsets count pixels: level l starts at off_l = sum over 1 <= k < l of N (H >> k) (W >> k), image i of it at
 * off_l + i (H >> l) (W >> l); the allocation holds off_L pixels, 3 floats each.
 *
 * Value of pixel (Y, X), channel c of level l >= 1, with s = 2^l (bit-exact recipe):
 *   S     = sum over the s x s pixels (Y s + dy, X s + dx) of level 0 of  c8 * a8 + 255 * (255 - a8)     (integers; a8 = alpha)
 *   value = (float)S / (float)(65025 * s * s)                                                         (one fp32 division)
 * S <= 65025 * 256 = 16,646,400 < 2^24 for s <= 16, so both operands are exact in fp32 and value is the correctly rounded box
 * average of the white-blended colours c/255 * a/255 + (1 - a/255): that is where the limit of 5 levels comes from.  Every level
 * is computed from level 0, never from the level above: no rounding compounds.  No atomics; one lane per output pixel.
 * Level 0 keeps the fp32 blend written above the single-scale sampler (three roundings); it can differ from S / 65025 by an ulp.
 *
 * Camera of level l: the pose of the image and the intrinsics (fx, fy, cx, cy) / 2^l, exact in fp32.  Pixel (y, x) of level l
 * then covers the pixels (y s .. y s + s - 1, x s .. x s + s - 1) of level 0, and its pixel_area, from the same device function
 * as every other ray of this library, is 4^l times a level-0 pixel's to first order in the pixel's angular size. */
#define RSN_PYRAMID_MAX_LEVELS 5

/* The levels 1 .. levels-1 of all images into `pyramid` (capacity pyramid_pixels >= off_L pixels, else an argument error); one
 * launch.  levels == 1 launches nothing and reads no pointer. */
int rsn_build_pyramid(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images, float* pyramid,
                      size_t pyramid_pixels, void* stream);

/* One training batch drawn across the levels, each level with probability 1/L (mip-NeRF draws uniformly over the pixels of all
 * scales and weights a ray's loss by 4^l; equal level probability is that objective by importance sampling, with unit weights).
 * Ray r (bit-exact recipe), with the Philox keying of the single-scale sampler:
 *   (u, v, -, -) = Philox4x32-10(counter = (step, r, 0, 0), key = (seed, rank))
 *   l = (uint32)(((uint64)v * L) >> 32);  H_l = H >> l, W_l = W >> l
 *   flat = (uint32)(((uint64)u * (N*H_l*W_l)) >> 32);  i = flat / (H_l*W_l);  y = (flat % (H_l*W_l)) / W_l;  x = flat % W_l
 * The ray is that of pixel (y, x) of the level's camera; rgb is the single-scale sampler's blend of images for l = 0 and the
 * pyramid's value for l >= 1.  Outputs as the single-scale sampler's, indices = (i, y, x) in the level's own pixel coordinates,
 * plus level int32 [R].  With levels == 1 (pyramid may be NULL) every output byte equals the single-scale sampler's. */
int rsn_sample_pyramid_rays(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                            const float* pyramid, size_t pyramid_pixels, const float* c2w, float fx, float fy, float cx,
                            float cy, int32_t n_rays, uint32_t seed, uint32_t rank, uint32_t step, float* origins,
                            float* directions, float* pixel_area, float* rgb, int32_t* indices, int32_t* level, void* stream);


/* ---- captures (additive to ABI 18: no existing call changes): image sets whose every image has its own camera, with lens
 * distortion -- what a nerfstudio-format transforms.json of real photographs describes.
 *
 * Camera table: cameras is fp32 [N, 9] on the device; row i = (fx, fy, cx, cy, k1, k2, k3, p1, p2) of image i.
 *
 * Model: COLMAP's / OpenCV's (COLMAP writes the coefficients of a transforms.json).  Image coordinates: x right, y DOWN.  For
 * the undistorted normalised point (X, Y):
 *   r2  = X^2 + Y^2
 *   rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *   Xd  = X rad + 2 p1 X Y + p2 (r2 + 2 X^2)
 *   Yd  = Y rad + p1 (r2 + 2 Y^2) + 2 p2 X Y
 *   u   = fx Xd + cx,   v = fy Yd + cy                                                                   (pixel coordinates)
 * (nerfstudio 0.3 undistorts the coordinates after its y flip, which amounts to -p1; this library does not: DESIGN.md 4.23.)
 *
 * Ray of pixel (y, x): (Xd, Yd) = ((x+.5-cx)/fx, (y+.5-cy)/fy); (X, Y) solves the model by Newton on the 2 x 2 system, started at
 * (Xd, Yd): exactly 10 iterations, no early exit, an iteration whose |det J| <= 1e-12 leaves the point where it is; the solve runs
 * in fp64.  Camera-space direction v = (X, -Y, -1); directions = normalize(c2w[:, :3] v); origins = c2w[:, 3].  pixel_area =
 * |d - d_x1| * |d - d_y1| as in the standalone data path; the x+1 / y+1 neighbours are undistorted by their own solves, their
 * camera-space offsets from v are differences of the solved points formed in fp64 and rounded to fp32 once, and the differences of
 * the unit vectors keep the cancellation-free rearrangement.  Nothing on the device checks that the solve converged: the caller
 * makes sure the model is invertible over the image (data.load_nerfstudio_split does) and that fx, fy != 0.
 *
 * A row whose five coefficients are all exactly zero runs the pinhole function of the standalone data path unchanged: its rays
 * have the bits rsn_camera_rays_image / rsn_sample_camera_rays give for the same (pose, intrinsics, y, x).
 *
 * Level l of a pyramid: the row's fx, fy, cx, cy over 2^l (exact); the coefficients act on normalised coordinates and stay. */

/* rsn_sample_pyramid_rays with a camera table in place of the four intrinsics: the same Philox recipe for level, image and pixel,
 * the same rgb and outputs, one launch, no atomics; image i's rays go through row i.  levels == 1 with pyramid NULL is the
 * single-scale batch: level may then be NULL too (where given it is written: zeros). */
int rsn_sample_capture_rays(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                            const float* pyramid, size_t pyramid_pixels, const float* c2w, const float* cameras, int32_t n_rays,
                            uint32_t seed, uint32_t rank, uint32_t step, float* origins, float* directions, float* pixel_area,
                            float* rgb, int32_t* indices, int32_t* level, void* stream);

/* rsn_camera_rays_image for ONE camera row (camera: device fp32 [9], read on the device): the sampler's device function, so equal
 * (i, y, x) give equal bits. */
int rsn_capture_rays_image(int32_t height, int32_t width, const float* c2w, const float* camera, float* origins,
                           float* directions, float* pixel_area, void* stream);


/* ---- captures: masks and fisheye lenses (additive to ABI 18: no existing call changes, and the calls above keep their bits).
 *
 * Camera table with 12 columns: row i = (fx, fy, cx, cy, k1, k2, k3, p1, p2, k4, model, 0).  model == 0: a perspective row, the
 * arithmetic of the 9-column table above on its first nine columns (k4 is not read).  model != 0 (the loader writes 1): OpenCV's
 * equidistant fisheye model, as COLMAP's OPENCV_FISHEYE writes it (p1, p2 are not read).  A call that takes camera_stride accepts
 * 9 (every row perspective) or 12.
 *
 * Fisheye ray of pixel (y, x), every step up to the rounding of the direction in fp64:
 *   (xd, yd) = ((x+.5-cx)/fx, (y+.5-cy)/fy);   theta_d = sqrt(xd^2 + yd^2)
 *   theta solves  theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d  by Newton from theta = theta_d:
 *     t2 = theta^2;  f  = theta (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))) - theta_d
 *                    f' = 1 + t2 (3 k1 + t2 (5 k2 + t2 (7 k3 + t2 9 k4)));   theta -= f / f'
 *     exactly 10 steps, none skipped early; a step with |f'| <= 1e-12 leaves theta where it is; then theta = min(max(theta, 0), pi)
 *   v = (xd s, -(yd s), -cos theta) with s = sin(theta) / theta_d;  at theta_d == 0:  v = (0, 0, -1)        (fp64 sin, cos, sqrt)
 * v is the camera-space UNIT direction; it is rounded to fp32 once.  The x+1 and y+1 neighbours get their own solves; their
 * camera-space offsets e = v_neighbour - v are formed in fp64 and rounded to fp32 once.  From there on fp32, as every other ray:
 * w = R v and g = R e with all three components (v.z > 0 beyond 90 degrees from the axis), directions = w / |w|, origins =
 * c2w[:, 3], pixel_area by the cancellation-free rearrangement of the standalone data path.  Nothing on the device checks that the
 * solve converged: the caller makes sure the model is invertible over the image (data.load_nerfstudio_split does).
 * Level l of a pyramid: the row's fx, fy, cx, cy over 2^l (exact); k1 .. k4 act on angles and stay.
 *
 * Live-pixel lists: masks is uint8 [N, H, W], non-zero = the pixel may be trained on.  Pixel (i, y, x) of level l has the flat
 * index i (H >> l)(W >> l) + y (W >> l) + x -- the numbering the samplers draw in -- and is live when ALL 2^l x 2^l level-0
 * pixels under it are, so that the pyramid's box colour of a live pixel never mixes a masked one in.  The list of a level holds
 * its live indices in ascending order; the lists are concatenated in level order, counts[l] is the length of level l's. */
#define RSN_LIVE_TILE 256          /* level pixels per workgroup of the compaction */
#define RSN_LIVE_SCAN_CHUNK 65536  /* level pixels per trip of the scan's loop: RSN_LIVE_TILE tiles; a carry crosses each boundary */

/* Bytes of workspace rsn_build_live_pixels needs (4 per tile of RSN_LIVE_TILE pixels of every level), or 0 with a message for a
 * shape rsn_build_pyramid would refuse. */
size_t rsn_live_pixels_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t levels);

/* counts (device uint32 [levels]) receives the lengths of the lists.  live == NULL (or live_capacity == 0): that is all.  Else
 * the lists are written to live (device uint32), but only entries < live_capacity: never a byte past it.  Stable compaction, no
 * atomics: per-tile counts, one workgroup per level scans them, every tile writes behind its own offset; two runs give the same
 * bytes, equal to numpy.flatnonzero of the level's liveness.  workspace: 4-byte aligned, device.  No host read, no allocation. */
int rsn_build_live_pixels(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* masks, uint32_t* live,
                          size_t live_capacity, uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* rsn_sample_capture_rays with two changes.  (a) With live != NULL the flat pixel of ray r at level l is
 *   live[live_offsets[l] + (uint32)(((uint64)u * count_l) >> 32)],   count_l = live_offsets[l+1] - live_offsets[l]
 * in place of (uint32)(((uint64)u * (N H_l W_l)) >> 32); live_offsets is device uint32 [levels + 1], the running sum of the counts
 * above.  live == NULL: every pixel, and live_offsets is not read.  A level with count_l == 0 is the caller's error; the kernel
 * then takes the level's pixel 0 and reads nothing outside the lists, and a list entry beyond the level's last pixel is clamped to
 * it.  (b) The camera row is read at camera_stride, and a fisheye row takes the fisheye ray.  The level draw (v), the gather, the
 * blend, the outputs and the Philox counter layout are unchanged: with live == NULL (or all pixels live) and perspective rows the
 * output bytes are rsn_sample_capture_rays'. */
int rsn_sample_capture_rays_live(int32_t n_images, int32_t height, int32_t width, int32_t levels, const uint8_t* images,
                                 const float* pyramid, size_t pyramid_pixels, const float* c2w, const float* cameras,
                                 int32_t camera_stride, const uint32_t* live, const uint32_t* live_offsets, int32_t n_rays,
                                 uint32_t seed, uint32_t rank, uint32_t step, float* origins, float* directions, float* pixel_area,
                                 float* rgb, int32_t* indices, int32_t* level, void* stream);

/* rsn_capture_rays_image for a row of camera_stride (9 or 12) columns: the sampler's device function, so equal (pose, row, y, x)
 * give equal bits; a perspective row gives rsn_capture_rays_image's. */
int rsn_capture_rays_image2(int32_t height, int32_t width, const float* c2w, const float* camera, int32_t camera_stride,
                            float* origins, float* directions, float* pixel_area, void* stream);


/* ---- mesh export: the iso-surface of a scalar volume as an indexed triangle mesh (additive to ABI 18: no existing call
 * changes).  Marching tetrahedra on the Kuhn (Freudenthal) split of every grid cell: no case table, consistent across
 * shared cell faces by construction (a surface away from the grid boundary is closed), and every surface vertex lies on
 * exactly one grid edge, so vertices are welded by arithmetic.  No atomics: two runs give the same bits in the same order.
 *
 * Grid: vol is fp32 [nz, ny, nx], x fastest; vertex (i, j, k) has flat index v = (k*ny + j)*nx + i and position
 * origin + spacing * (i, j, k) (per axis: one fp32 multiply, one fp32 add).  Vertex v owns 7 outgoing edges dir = 0..6
 * towards the offsets (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1); an edge exists if its far end is in
 * the grid.  The cell with lowest corner c splits into 6 tetrahedra, one per permutation (a, b, c') of the axes, with
 * vertices c, c + e_a, c + e_a + e_b, c + (1,1,1).
 *
 * Classification: a vertex is inside when vol >= iso (NaN: outside).
 * Surface vertices: one per existing edge whose ends differ, numbered in ascending (v, dir).  With lo = v the owning
 *   (lower-index) end and hi the far end: t = (iso - f_lo) / (f_hi - f_lo), a NaN t becomes 0.5, then t is clamped to
 *   [0, 1]; p = p_lo + t * (p_hi - p_lo) per axis, clamped to [p_lo, p_hi]: finite and on the edge for any input bits.
 * Triangles: a tetrahedron with 1 or 3 inside vertices gives one, with 2 inside two; the right-hand normal points to
 *   the outside (towards lower values).  Order: ascending cell (flat index of its lowest corner), then the permutations
 *   in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx, then within a tetrahedron with vertices q = 0..3 in the order
 *   above: one vertex i alone on its side, the others j < k < l: (e_ij, e_ik, e_il); inside a < b, outside c < d:
 *   (e_ac, e_ad, e_bd) then (e_ac, e_bd, e_bc); in both cases the last two entries swap when the orientation asks for it.
 *
 * The workspace-size call returns the bytes the other two need (5 per grid point + 8 per 1024 points), or 0 with a
 * message for dimensions outside the limits: every dimension >= 2 (else RSN_ERR_INVALID_ARGUMENT from the other two)
 * and nx*ny*nz <= 2^27 (else RSN_ERR_UNSUPPORTED), so that 8*v + dir and 12 triangles per cell fit an int32.
 * The count call classifies, scans and leaves in `workspace` (4-byte aligned) what the emit call needs for the same
 * vol and iso; counts (device, [2]) receives the numbers of vertices and triangles.
 * The emit call writes positions [V,3], vert_key [V] = 8*v + dir (or NULL) and triangles [T,3] (vertex ids), but only
 * vertices < max_vertices and triangles < max_triangles: never a byte past either capacity; an output with capacity 0
 * may be NULL, and with both capacities 0 nothing is launched.  origin3 / spacing3 are HOST arrays (spacing > 0). */
size_t rsn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int rsn_mesh_count(int32_t nx, int32_t ny, int32_t nz, const float* vol, float iso, void* workspace, size_t workspace_bytes,
                   int32_t* counts, void* stream);
int rsn_mesh_emit(int32_t nx, int32_t ny, int32_t nz, const float* vol, float iso, const float* origin3,
                  const float* spacing3, const void* workspace, size_t workspace_bytes, int32_t max_vertices,
                  int32_t max_triangles, float* positions, int32_t* vert_key, int32_t* triangles, void* stream);


/* ---- TSDF fusion: depth maps of posed pinhole cameras into a truncated signed distance volume (additive to ABI 18: no existing
 * call changes).  The volume is what the mesh calls extract from: a mesh of the surface the model's own depth maps describe.
 *
 * Grid: tsdf and weight are fp32 [nz, ny, nx] in the layout of the mesh calls (x fastest, vertex (i, j, k) at
 * origin + spacing * (i, j, k)); origin3 / spacing3 are HOST arrays.  Cameras: c2w fp32 [n_views,3,4] (row-major, device) and one
 * set of intrinsics, in the ray convention written above rsn_sample_camera_rays; depth fp32 [n_views, height*width] (device),
 * row-major, the EUCLIDEAN distance along the ray of pixel (y, x) -- the model's median depth depth_fine, from which it starts its
 * own reflected rays.  There is no accumulation input: the median depth of a ray that does not reach 0.5 opacity is its last
 * sample, so such a ray carves free space up to its far end.
 *
 * Views are applied in ascending view order at every grid vertex, so a call with n views equals n calls of one view, bit for bit;
 * the caller batches views only to bound the memory its depth maps hold.  Per vertex (T = tsdf, W = weight) and view, every step
 * one correctly rounded fp32 operation in exactly this order:
 *   p_a   = o_a + s_a * idx_a                                            a = 0, 1, 2
 *   q_a   = p_a - c2w[a][3]
 *   cam_c = (c2w[0][c]*q_0 + c2w[1][c]*q_1) + c2w[2][c]*q_2              c = 0, 1, 2
 *   z     = -cam_2; the view is skipped unless z > 0
 *   u     = (fx*cam_0)/z + cx,  v = cy - (fy*cam_1)/z                    the inverse of the ray convention: the pixel whose square
 *                                                                        holds the projection is x = floor(u), y = floor(v)
 *   skipped unless 0 <= u < width and 0 <= v < height, compared as floats (a NaN skips)
 *   r     = sqrt((q_0*q_0 + q_1*q_1) + q_2*q_2); skipped if r < near
 *   D     = depth[view][y*width + x]; skipped if D is not finite
 *   s     = D - r; skipped if s < -trunc: the vertex is hidden behind the surface this view saw
 *   d     = min(1, s / trunc)
 *   Wn    = W + 1;  T = (T*W + d) / Wn;  W = Wn
 * A skipped view leaves both words of that vertex untouched.  T is positive in front of the surface, up to 1 in free space, and
 * negative down to -1 behind it; W counts the views that reached the vertex.
 *
 * RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): a dimension below 2; height < 1, width < 1 or
 * height*width > 2^31 - 1; n_views < 0; a NULL pointer when n_views > 0; trunc not finite or <= 0; near not finite; fx or fy not
 * finite or zero.  RSN_ERR_UNSUPPORTED for nx*ny*nz > 2^27.  n_views == 0 launches nothing.  No allocation and no synchronisation;
 * depth is indexed in 64 bits.  No atomics: every word has one owner, so the result is deterministic. */
int rsn_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* origin3, const float* spacing3, int32_t n_views,
                       const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx, float cy, const float* depth,
                       float trunc, float near, float* tsdf, float* weight, void* stream);


/* ---- visualisation: per-pixel floats as one 8-bit RGB tile of a panel (additive to ABI 18: no existing call changes).
 * One call draws one channel of a rendered view into one tile, so a frame is a handful of launches on the caller's stream.
 *
 * out is uint8 [height, pitch, 3] with pitch in pixels; input pixel p = y*width + x goes to out[(y*pitch + x0 + x)*3 + c],
 * c = 0..2, and no byte outside the tile [x0, x0 + width) of any row is written.  Every step below is one fp32 operation:
 *   sat(v)  = 0 if v is NaN or v <= 0, 1 if v > 1, else v   (-inf -> 0, +inf -> 1, -0.0 -> +0)
 *   a       = sat(alpha[p]), or 1 when alpha is NULL
 *   over(c) = c*a + (1 - a)            white beneath: what RGBRenderer does with the model's white background and
 *                                      nerfstudio's apply_depth_colormap with its accumulation; a multiply, a subtract, an add
 *   q(v)    = (uint8)(int)(v*255.0f + 0.5f) for v in [0, 1]      (the quantisation of the trainer's eval panels)
 * RSN_VIS_RGB : x [N,3]; out_c = q(over(sat(x_c)))
 * RSN_VIS_UNIT: x [N,3]; out_c = q(over(sat(x_c*0.5f + 0.5f)))   (the usual colouring of a unit normal)
 * RSN_VIS_GRAY: x [N];   t = sat((x - lo) / (hi - lo)), all three channels q(over(t))
 * RSN_VIS_LUT : x [N];   t as above, k = (int)(t*255.0f), in [0, 255] since t <= 1; out_c = q(over(lut[k][c])) with lut an
 *               fp32 [256,3] table on the device, values in [0, 1].  With the turbo table, lo / hi = near / far and alpha =
 *               the accumulation this is nerfstudio 0.3 colormaps.apply_depth_colormap, except that nerfstudio divides by
 *               (far - near + 1e-10) and this call by (hi - lo).
 * lo / hi / lut are not read by the kinds that do not name them.
 * RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): height < 1, width < 1 or height*width >
 * 2^31 - 1; x0 < 0 or x0 + width > pitch; an unknown kind; x or out NULL; lut NULL with RSN_VIS_LUT; for GRAY and LUT lo or
 * hi not finite, or hi <= lo.  No allocation and no synchronisation. */
#define RSN_VIS_RGB 0
#define RSN_VIS_UNIT 1
#define RSN_VIS_GRAY 2
#define RSN_VIS_LUT 3
int rsn_visualize(int32_t height, int32_t width, int32_t kind, const float* x, const float* alpha, float lo, float hi,
                  const float* lut, uint8_t* out, int32_t pitch, int32_t x0, void* stream);


/* ---- occupancy: skip the rays of an eval render that see nothing (additive to ABI 18: no existing call changes).
 *
 * Grid: nx * ny * nz vertices in the layout of the mesh calls (x fastest, vertex (i, j, k) at origin + spacing * (i, j, k)) and
 * (nx-1)(ny-1)(nz-1) cells; cell (i, j, k) spans the vertices (i..i+1, j..j+1, k..k+1), has flat index
 * c = (k*(ny-1) + j)*(nx-1) + i and is bit c % 32 of uint32 word c / 32.  rsn_occupancy_bytes: the size of that bit array, the word
 * count rounded up times 4; 0 with a message when a dimension is below 2 or nx*ny*nz > 2^27.
 *
 * rsn_occupancy_build: bits from a density volume vol (fp32 [nz, ny, nx]).  Cell (i, j, k) is occupied if and only if some vertex
 * (i', j', k') inside the grid has !(vol < threshold) -- so a NaN vertex counts as occupied -- with i - dilate <= i' <= i + 1 + dilate
 * and likewise for j and k; dilate = 0, 1 or 2.  That is "any of the cell's eight corners, then grown by `dilate` cells in the
 * Chebyshev sense", stated over vertices so that no temporary bit array is needed.  The unused high bits of the last word are written
 * as 0; `bytes` is the capacity of bits (at least rsn_occupancy_bytes, else RSN_ERR_INVALID_ARGUMENT) and no byte past the bit array
 * is written.  Bit-exact and deterministic.
 *
 * rsn_occupancy_cull: which of n_rays segments o + t d, t in [near, far] (origins / directions [R,3], nears / fars [R]; d as given,
 * not normalised) can be skipped.  origin3 / spacing3 are HOST arrays (finite, spacing > 0).  hit[r] (uint8) = 1 when the segment
 * crosses an occupied cell; with outside_occupied != 0 also when any part of it lies outside the grid's box; and always when an
 * origin, direction, near or far is not finite or far < near: a ray that cannot be reasoned about is never culled.  The decision is
 * exact up to a band of 1e-3 of a cell around the cell faces (and the box's), inside which either answer may come; it is
 * deterministic.  n_hit (device int32) = the number of hit rays; ray_index (int32 [R]) is a permutation of 0..R-1: first the hit
 * rays in ascending order, then the culled rays in ascending order (a stable compaction without atomics; `workspace`: device memory
 * of rsn_occupancy_cull_workspace_bytes(n_rays) bytes, contents irrelevant).  n_rays == 0 launches nothing and sets *n_hit = 0.
 *
 * rsn_scatter_rows: results of the compacted rays back to their rows: out[ray_index[i]*row_floats + c] = src[i*row_floats + c] when
 * i < *n_dev (n_dev NULL: n_rows), `fill` otherwise, for i < n_rows, c < row_floats.  With ray_index a permutation of 0..n_rows-1
 * every row of out is written exactly once; rows of src at and past the count are never read, and an entry of ray_index outside
 * 0..n_rows-1 writes nothing. */
size_t rsn_occupancy_bytes(int32_t nx, int32_t ny, int32_t nz);
int rsn_occupancy_build(int32_t nx, int32_t ny, int32_t nz, const float* vol, float threshold, int32_t dilate, uint32_t* bits,
                        size_t bytes, void* stream);
size_t rsn_occupancy_cull_workspace_bytes(int32_t n_rays);
int rsn_occupancy_cull(int32_t n_rays, const float* origins, const float* directions, const float* nears, const float* fars,
                       int32_t nx, int32_t ny, int32_t nz, const float* origin3, const float* spacing3, const uint32_t* bits,
                       int32_t outside_occupied, uint8_t* hit, int32_t* n_hit, int32_t* ray_index, int32_t* workspace,
                       void* stream);
int rsn_scatter_rows(int32_t n_rows, const int32_t* n_dev, const int32_t* ray_index, const float* src, int32_t row_floats,
                     float fill, float* out, void* stream);

/* ---- occupancy, per sample: evaluate the field only on the samples of a level that lie in occupied cells (additive to ABI 18).
 *
 * A level has n_rays rays of n_samples intervals, euclid_bins [R,S+1]; sample i of ray r is point p = r*S + i, as in
 * rsn_field_forward_frustum.  rsn_occupancy_compact_samples decides which samples are live and lists them as "rays" of one sample
 * each, which rsn_field_forward_frustum evaluates with n_samples = 1, euclid_bins = bins_c and n_dev = n_live; rsn_scatter_level
 * writes the results back to their [R,S] slots.  The grid arguments (nx .. outside_occupied) are those of rsn_occupancy_cull.
 *
 * rsn_occupancy_samples_workspace_bytes: HOST only; 0 with a message when n_rays < 0, n_samples < 1 or n_rays * n_samples * 3 does
 * not fit in int32 (rsn_occupancy_compact_samples refuses the same shapes with RSN_ERR_INVALID_ARGUMENT).
 *
 * rsn_occupancy_compact_samples, the rules:
 *  - live[p] (uint8 [R*S]) = 0 for r >= *n_dev (n_dev NULL: n_rays; clamped to 0 .. n_rays); the inputs of those rays are never read.
 *  - Otherwise live[p] = 1 when at least one of these holds, else 0:
 *      (a) the sub-segment o + t d, t in [bins[r,i], bins[r,i+1]], is a hit by exactly the predicate of rsn_occupancy_cull: the same
 *          1e-3-cell band, the same outside_occupied, and the same "never skip what cannot be reasoned about" clauses, which cover a
 *          non-finite origin, direction or bin and bins[r,i+1] < bins[r,i];
 *      (b) the cone is wider than the grid's margin: bins[r,i+1] * |d| * sqrt(pixel_area[r] / pi) > max_radius, evaluated in fp64
 *          (sqrt(pixel_area) / sqrt(pi) is the cone's radius at unit distance; a pixel_area below 0 never satisfies it);
 *      (c) pixel_area[r] is not finite.
 *    max_radius = +inf switches (b) off; NaN is RSN_ERR_INVALID_ARGUMENT.
 *  - n_live (device int32) = the number of live samples.
 *  - sample_index (int32 [R*S]) is a permutation of 0 .. R*S-1: the live samples in ascending order, then the others in ascending
 *    order -- the contract of ray_index: stable, no atomics, deterministic.
 *  - For j < *n_live, row j of origins_c [R*S,3], directions_c [R*S,3], pixel_area_c [R*S] and bins_c [R*S,2] (8-byte aligned)
 *    holds the origin, direction and pixel area of the ray of sample sample_index[j] and its (t_i, t_i+1), bit for bit.  Rows at and
 *    past *n_live are left unwritten.
 *  - n_rays == 0 launches nothing and sets *n_live = 0.  workspace: device memory of rsn_occupancy_samples_workspace_bytes bytes,
 *    contents irrelevant.  No allocation, no synchronisation, no host read.
 *
 * rsn_scatter_level: one launch for every non-NULL member of src (rows of 1 or 3 floats, n_points rows each): row j of a member of
 * src goes to row sample_index[j] of the same member of dst for j < *n_live (clamped to 0 .. n_points), and every row of dst that
 * belongs to no live sample is written as zeros -- a zero sigma gives a zero weight, so no other member of a skipped sample reaches
 * a ray's result.  With sample_index a permutation every row of dst is written exactly once; an entry outside 0 .. n_points-1
 * writes nothing; rows of src at and past *n_live are never read.  A member set in one struct and NULL in the other is
 * RSN_ERR_INVALID_ARGUMENT. */
size_t rsn_occupancy_samples_workspace_bytes(int32_t n_rays, int32_t n_samples);
int rsn_occupancy_compact_samples(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* origins,
                                  const float* directions, const float* pixel_area, const float* euclid_bins, int32_t nx, int32_t ny,
                                  int32_t nz, const float* origin3, const float* spacing3, const uint32_t* bits,
                                  int32_t outside_occupied, float max_radius, uint8_t* live, int32_t* n_live, int32_t* sample_index,
                                  float* origins_c, float* directions_c, float* pixel_area_c, float* bins_c, int32_t* workspace,
                                  void* stream);
int rsn_scatter_level(int32_t n_points, const int32_t* n_live, const int32_t* sample_index, const rsn_field_outputs* src,
                      const rsn_field_outputs* dst, void* stream);


/* ---- point cloud: depth maps of posed pinhole cameras into one deduplicated, deterministically ordered set of points (additive to
 * ABI 18: no existing call changes).  A point is where the model starts a reflected ray: origin + depth * direction of a pixel.
 *
 * Inputs, in the layouts of rsn_tsdf_integrate: c2w fp32 [n_views,3,4] (row-major, device) and one set of intrinsics height, width,
 * fx, fy, cx, cy; depth fp32 [n_views, height*width] (device), row-major, the EUCLIDEAN distance along the ray; accumulation fp32
 * [n_views, height*width] (device) or NULL; view0 >= 0, the number of views that earlier calls have already processed.  A grid of
 * nx * ny * nz CELLS, every dimension >= 1, with origin3 / spacing3 as HOST arrays: cell (i, j, k) spans
 * origin + spacing * (i..i+1, j..j+1, k..k+1) and has flat index (k*ny + j)*nx + i.
 *
 * Global pixel index: pixel (y, x) of view v of a call has g = ((view0 + v)*height + y)*width + x; (view0 + n_views)*height*width
 * must not exceed 2^31 - 1.
 *
 * The ray (o, d) of a pixel is the one written above rsn_sample_camera_rays, from the same device function that call and
 * rsn_camera_rays_image run: equal (pose, intrinsics, y, x) give bit-identical rays.
 *
 * Candidate rule.  Pixel p = y*width + x of view v is a candidate if and only if all of the following hold; every arithmetic step
 * is one correctly rounded fp32 operation, none contracted into a fused multiply-add:
 *   1. D = depth[v][p] is finite and D > 0.
 *   2. accumulation is NULL, or accumulation[v][p] >= min_accumulation (a NaN fails).
 *   3. For each of the up to four neighbours (y-1, x), (y+1, x), (y, x-1), (y, x+1) inside the image of the same view whose depth
 *      Dn is finite: NOT fabsf(D - Dn) > edge * fminf(D, Dn) -- one subtract, one multiply, one compare.  edge = +inf switches the
 *      test off (a NaN product compares false).  The neighbour's accumulation plays no part, so a silhouette pixel next to a ray
 *      that ran to its far end is rejected: that is the point of the test.
 *   4. The point lies inside the grid:  t_a = D * d_a,  p_a = o_a + t_a,  q_a = (p_a - origin_a) / spacing_a  for a = 0, 1, 2, and
 *      0 <= q_a < n_a on all three axes, compared as floats with n_a converted to float (a NaN fails).  cell_a = (int)floorf(q_a).
 *
 * rsn_pointcloud_workspace_bytes: HOST only; the bytes rsn_pointcloud_select needs for a call of this shape (8 per 256 pixels + 1
 * per pixel, rounded up), never 0 for a valid shape; 0 with a message when n_views < 0, height < 1, width < 1 or
 * n_views*height*width > 2^31 - 1.
 *
 * rsn_pointcloud_mark: owner is int32 [nz, ny, nx] on the device, filled by the caller with 0x7fffffff before the first call.  For
 * every candidate, owner[cell] = min(owner[cell], g) by an integer atomic minimum -- the only atomic of these calls; an integer
 * minimum does not depend on the order, so owner is deterministic.  owner == NULL means no thinning: evaluating the rule would
 * leave no trace, so the call checks its arguments and launches nothing.
 *
 * rsn_pointcloud_select: a candidate is KEPT if and only if owner == NULL or owner[cell] == g.  *n_points (device int32) = the
 * number of kept pixels of this call; rows 0 .. *n_points-1 of pixel_index (int32 [n_views*height*width]) hold the kept pixels' g
 * in ascending order and the same rows of positions (fp32 [n_views*height*width, 3]) their (p_0, p_1, p_2), bit for bit.  Rows at
 * and past the count are left unwritten.  The compaction is stable and uses no atomics, as in rsn_occupancy_cull.  workspace:
 * device memory of at least rsn_pointcloud_workspace_bytes bytes, 4-byte aligned, contents irrelevant (RSN_ERR_WORKSPACE when
 * workspace_bytes is less).  n_candidates (device int32, or NULL) receives the number of candidates of this call, before the owner
 * test; without an owner it equals *n_points.  n_views == 0 launches nothing and sets both counts to 0; n_points must never be NULL.
 * Cost: two passes over the pixels and, between them, one workgroup that scans the counts of the tiles of 256 pixels, 256 tiles per
 * step -- a serial term of n_views*height*width / 65536 steps, 78 for eight 800 x 800 views and 32768 at the largest shape.
 *
 * Two properties follow.  A later call has higher g, so it never takes a cell from an earlier one: views 0..n-1 in one mark + select
 * pair keep exactly the pixels, in exactly the order, of any split into consecutive pairs that share owner and advance view0 (the
 * rows of the pairs concatenated).  And with thinning every cell that holds a candidate gets exactly one point, its candidate with
 * the lowest g.
 *
 * Both calls: RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): a grid dimension below 1; height or
 * width below 1; n_views < 0 or view0 < 0; the index bound above exceeded; fx or fy not finite or zero; min_accumulation NaN; edge
 * NaN or negative; a NULL c2w, depth, origin3 or spacing3 when n_views > 0 (and for select a NULL workspace, pixel_index or
 * positions); a spacing that is not finite or not positive, or an origin that is not finite.  RSN_ERR_UNSUPPORTED for
 * nx*ny*nz > 2^27.  No allocation, no synchronisation and no host read. */
size_t rsn_pointcloud_workspace_bytes(int32_t n_views, int32_t height, int32_t width);
int rsn_pointcloud_mark(int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                        const float* depth, const float* accumulation, int32_t view0, int32_t nx, int32_t ny, int32_t nz,
                        const float* origin3, const float* spacing3, float min_accumulation, float edge, int32_t* owner,
                        void* stream);
int rsn_pointcloud_select(int32_t n_views, const float* c2w, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                          const float* depth, const float* accumulation, int32_t view0, int32_t nx, int32_t ny, int32_t nz,
                          const float* origin3, const float* spacing3, float min_accumulation, float edge, const int32_t* owner,
                          void* workspace, size_t workspace_bytes, int32_t* n_points, int32_t* n_candidates, int32_t* pixel_index,
                          float* positions, void* stream);


/* ---- decimation: an indexed triangle mesh reduced by vertex clustering (additive to ABI 18: no existing call changes).  A regular
 * grid of cluster cells covers a box; all vertices in a cell merge into one; triangles that collapse disappear.  The result is
 * stated step by step so that a numpy restatement reproduces it by bits (tests/decimate_reference.py).
 *
 * Inputs: positions fp32 [n_vertices,3] and triangles int32 [n_triangles,3] on the device; origin3 / cell3 HOST arrays; cx, cy, cz
 * CELLS per axis, each >= 1, cx*cy*cz <= 2^27: cell (i, j, k) spans origin + cell * (i..i+1, j..j+1, k..k+1) and has the flat id
 * (k*cy + j)*cx + i -- the frame of the point-cloud calls (n cells, n intervals).
 *
 * Cell of a vertex, per axis a with n = the cell count of the axis, every step one correctly rounded fp32 operation:
 *   1. u = (p_a - o_a) / c_a: one subtract, one divide.  A non-finite u (NaN or an infinity) becomes 0.
 *   2. i = floor(u), clamped to [0, n - 1].  A vertex on an interior cell face belongs to the upper cell; a vertex on the box's upper
 *      face, or outside the box, to the nearest boundary cell.
 * Representative of a cell: the mean of EVERY input vertex that falls in it (whether a triangle names the vertex or not), in fixed
 * point, so that it does not depend on the order of arrival:
 *   3. f = u - (float)i in fp32;  q = rint(f * 2^20), ties to even, clamped to [0, 2^20].
 *   4. per cell and axis S_a = the 64-bit integer sum of the q, and m = the int32 number of vertices of the cell.
 *   5. in fp64, on the widened fp32 o_a and c_a:  r_a = o_a + c_a * ((double)i + ((double)S_a / (double)m) * 2^-20) -- one division,
 *      an exact scaling, one add, one multiply, one add, none contracted -- rounded once to fp32.
 * Integer atomic adds (the sums, the member counts and the four counts below) are the only atomics; there is no float atomic.
 *
 * Triangles.  Each corner maps to the cell of its vertex.  A triangle with an index outside [0, n_vertices) -- which is never
 * dereferenced -- or with two corners in one cell is DEGENERATE and dropped.  The others are grouped by the UNORDERED set of their
 * three cells.  Within a group a triangle is `+` when the cyclic order of its corners is that of the ascending cells, and `-`
 * otherwise.  With net = n_plus - n_minus the survivors of a group are the first |net| triangles, by original index, of the majority
 * orientation; net = 0 leaves none.  min(n_plus, n_minus) is the group's number of CANCELLED PAIRS, so that n_triangles = survivors
 * + degenerate + 2 * cancelled pairs.  This is not "drop duplicates": clustering is a simplicial map and keeps a cycle a cycle only
 * if opposite pairs cancel and multiplicity is kept; with it a closed input gives an output in which every directed edge (a, b)
 * occurs exactly as often as (b, a).  Manifoldness and the genus are NOT promised.
 *
 * Output.  Vertices: the cells a surviving triangle names, in ascending cell id, at their representative.  Triangles: the survivors
 * in ascending original index, each with its corners in its own order, renumbered to the new vertex ids.  Same bytes in the same
 * order from run to run.
 *
 * The calls, in this order on one stream, with one workspace (rsn_decimate_workspace_bytes for the same n_vertices, n_triangles and
 * cell counts, 8-byte aligned, contents irrelevant before the first call and kept by the caller between the calls) and one counts
 * array, int32 [5] on the device: [0] vertices out, [1] triangles out, [2] degenerate triangles, [3] cancelled pairs, [4] occupied
 * cells.
 *   rsn_decimate_cluster  zeroes counts; finds the cell of every vertex and the RANK of every occupied cell among the occupied
 *       cells in ascending id (counts[4] = their number); writes keys int64 [n_triangles]: for a triangle with ranks r0 < r1 < r2,
 *       r0 * 2^42 + r1 * 2^21 + r2; for a degenerate one 2^63 - 1, and counts[2] = their number.
 *   the caller sorts the keys STABLY in ascending order (signed 64-bit) and keeps the sorted keys and, as int64, the original index
 *       of every sorted entry (what torch.sort(keys, stable=True) returns).  It is the one step left to the caller.
 *   rsn_decimate_resolve  applies the group rule: counts[1] and counts[3].  Once per rsn_decimate_cluster call (it adds to the
 *       counts).  One lane walks a group, so its time grows with the largest number of triangles that share three cells.
 *       An entry of `order` outside [0, n_triangles) is skipped, never dereferenced.  Enough for a caller that only wants
 *       the number of survivors.
 *   rsn_decimate_count  numbers the surviving triangles and the cells they name: counts[0], and counts[1] again.  The caller reads
 *       counts once, here, to size the outputs -- as with rsn_mesh_count / rsn_mesh_emit.
 *   rsn_decimate_emit  sums the vertices of the named cells and writes out_positions fp32 [counts[0],3] and out_triangles int32
 *       [counts[1],3], but only vertices < max_vertices and triangles < max_triangles: never a byte past either capacity; an output
 *       with capacity 0 may be NULL, and with both capacities 0 nothing is launched.
 * The ranks must fit 21 bits.  The number of occupied cells is known on the device only and the library never reads it back: when
 * counts[4] exceeds 2^21 no triangle is grouped, counts[1..3] stay 0 and the caller must treat the call as refused
 * (RSN_ERR_UNSUPPORTED is what the package raises); nothing is written out of bounds.  min(n_vertices, cx*cy*cz) <= 2^21 rules it out.
 *
 * All calls: RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): a cell count below 1; a negative
 * n_vertices or n_triangles; with both counts positive a NULL workspace (or one not 8-byte aligned), positions, triangles, keys,
 * sorted_keys, order or counts, or an output with a capacity above 0; a NULL origin3 or cell3; an origin that is not finite; a cell
 * size that is not finite or not above 0; a negative capacity.  RSN_ERR_UNSUPPORTED for cx*cy*cz > 2^27 (the size call returns 0
 * with a message for these); RSN_ERR_WORKSPACE for a workspace_bytes below the size.  n_vertices == 0 or n_triangles == 0 launches
 * nothing: rsn_decimate_cluster then only zeroes counts.  No allocation, no synchronisation and no host read. */
size_t rsn_decimate_workspace_bytes(int32_t n_vertices, int32_t n_triangles, int32_t cx, int32_t cy, int32_t cz);
int rsn_decimate_cluster(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles,
                         const float* origin3, const float* cell3, int32_t cx, int32_t cy, int32_t cz, void* workspace,
                         size_t workspace_bytes, int64_t* keys, int32_t* counts, void* stream);
int rsn_decimate_resolve(int32_t n_vertices, int32_t n_triangles, int32_t cx, int32_t cy, int32_t cz, const int64_t* sorted_keys,
                         const int64_t* order, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream);
int rsn_decimate_count(int32_t n_vertices, int32_t n_triangles, const int32_t* triangles, int32_t cx, int32_t cy, int32_t cz,
                       void* workspace, size_t workspace_bytes, int32_t* counts, void* stream);
int rsn_decimate_emit(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles, const float* origin3,
                      const float* cell3, int32_t cx, int32_t cy, int32_t cz, void* workspace, size_t workspace_bytes,
                      int32_t max_vertices, int32_t max_triangles, float* out_positions, int32_t* out_triangles, void* stream);


/* ---- texture atlas: where on an indexed triangle mesh every texel of a per-triangle atlas samples the field (additive to ABI 18:
 * no existing call changes).  The field's material maps are then baked at those points, finer than the mesh's vertices.
 *
 * Layout.  One pair of triangles gets one square of P x P texels, P = texels >= 4 -- nerfstudio's "custom" per-triangle unwrap with
 * a gutter, so that bilinear filtering never mixes two triangles.  T triangles need S = ceil(T / 2) squares; with Q =
 * squares_per_row squares in a row (the caller's choice, 2*Q*Q >= T; the package takes Q = max(1, ceil(sqrt(S))) in integers) the
 * texture is N x N texels, N = Q*P, row-major with image row 0 at the top.  Texel (row, col) has flat index row*N + col and
 *   sx = col / P, a = col % P, sy = row / P, b = row % P;  square q = sy*Q + sx holds triangle 2q (lower) and 2q + 1 (upper).
 * Texel centres sit at integer (a, b).
 *                            lower triangle 2q                        upper triangle 2q + 1
 *   corners 0, 1, 2 at       (0,0), (P-3,0), (0,P-3)                  (P-1,P-1), (2,P-1), (P-1,2)
 *   owns the texels with     a + b <= P-2                             a + b >= P-1
 *   live if additionally     a <= P-3 and b <= P-3                    a >= 2 and b >= 2
 *   u                        (float)a / (float)(P-3)                  (float)(P-1-a) / (float)(P-3)
 *   v                        (float)b / (float)(P-3)                  (float)(P-1-b) / (float)(P-3)
 * A texel is UNUSED when it is owned but not live, when its triangle's index is >= T, or when any vertex index of its triangle lies
 * outside [0, V) -- then positions is not read for it.  An unused texel gets face = -1 and zeros in point and footprint.
 * A live texel of triangle t with vertices p0, p1, p2 = positions[triangles[t][0..2]] gets face = t and, per axis,
 *   w0 = (1 - u) - v,   p = (w0*p0 + u*p1) + v*p2
 *   h  = max(|p1 - p0|, |p2 - p0|) / (float)(P-3),   each length sqrt((dx*dx + dy*dy) + dz*dz)
 * in point and footprint; every difference, product, sum, quotient and square root is one correctly rounded fp32 operation, none
 * contracted into a fused multiply-add.  The live texels with u + v > 1 are the gutter: real samples slightly beyond the
 * hypotenuse, in the triangle's plane.  Two properties (tests/test_texture_cpu.py checks both): (a) every texel that bilinear
 * filtering reads with a weight above zero from a point inside a triangle's corner triangle is a live texel of that triangle;
 * (b) no texel is live for two triangles.  Corner k of a triangle at texel centre (col_k, row_k) has the OBJ coordinate
 * vt = ((col_k + 0.5) / N, 1 - (row_k + 0.5) / N).
 *
 * positions fp32 [n_vertices,3] and triangles int32 [n_triangles,3] on the device; face int32 [N*N], point fp32 [N*N,3], footprint
 * fp32 [N*N].  One lane per texel; every output word has one owner: no atomics, so two runs give the same bits; no allocation and
 * no synchronisation; no word outside the three outputs' N*N rows is written.  Degenerate triangles give finite outputs.
 * RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): texels < 4; squares_per_row < 1; n_vertices < 0
 * or n_triangles < 0; 2*squares_per_row^2 < n_triangles; with n_triangles > 0 a NULL triangles, face, point or footprint, or a NULL
 * positions when n_vertices > 0.  RSN_ERR_UNSUPPORTED for N > 16384.  n_triangles == 0 launches nothing. */
int rsn_texture_points(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles, int32_t texels,
                       int32_t squares_per_row, int32_t* face, float* point, float* footprint, void* stream);


/* ---- geometry metrics: the composited predicted normal of an eval view against a ground-truth normal map, and the accumulation
 * against the ground-truth alpha (additive to ABI 18: no existing call changes).  The numbers of the Ref-NeRF results table: the
 * alpha-weighted mean angular error in degrees (multinerf's compute_normal_mae), here with its error map, on the device.
 *
 * P = n_pixels.  normals fp32 [P,3] is the predicted row p of every pixel; it is NOT required to be of unit length (the angle does
 * not depend on the lengths, so nothing is normalised and the ground truth decodes exactly).  gt_normals uint8 [P,3] holds the
 * bytes u_c of a normal map, encoding n_c * 0.5 + 0.5; gt_rgba uint8 [P,4], of which only the alpha byte a (index 3) is read;
 * accumulation fp32 [P] or NULL; rotation fp32 [9], a row-major 3 x 3 matrix R on the device, or NULL; error_map fp32 [P] or NULL.
 * Per pixel, every step one correctly rounded fp32 operation unless said otherwise, none contracted into a fused multiply-add:
 *   1. v_c = 2*u_c - 255 in integers (an odd number in [-255, 255]), g_c = (float)v_c: exact.
 *   2. valid = a > 0 and max_c |v_c| > 1.  The bytes 127 and 128 in all three channels mean "no normal" (how a background is
 *      written: both decode to within half a step of zero); the test is on the integers, before any rotation.
 *   3. with rotation: g = R g, g'_r = (R[3r]*g_0 + R[3r+1]*g_1) + R[3r+2]*g_2 for r = 0, 1, 2 (all three from the unrotated g).
 *   4. c = p x g: c_0 = p_1*g_2 - p_2*g_1, c_1 = p_2*g_0 - p_0*g_2, c_2 = p_0*g_1 - p_1*g_0;
 *      s = sqrtf((c_0*c_0 + c_1*c_1) + c_2*c_2);  d = (p_0*g_0 + p_1*g_1) + p_2*g_2.
 *   5. theta = atan2f(s, d), in [0, pi]; but theta = (float)(pi/2) when s == 0 and d == 0, which is what a zero prediction gives
 *      (multinerf normalises with an epsilon and gets arccos(0) there).  deg = theta * (float)(180/pi).
 *      atan2 of the cross and the dot product is the angle multinerf takes as arccos of the normalised dot product; it is used
 *      because it is well conditioned at 0 and 180 degrees, where fp32 arccos loses half its digits -- and a good model sits at 0.
 *      A prediction so small or so large that the squares of step 4 leave the fp32 range is outside the recipe.
 *   6. error_map[i] = valid ? deg : 0.
 * Sums, in fp64, in an order fixed by (P, pixel index) alone (below):
 *   S1 = sum over the valid pixels of (double)a * (double)deg        S2 = sum over the valid pixels of a
 *   S3 = sum over ALL pixels of |(double)accumulation - (double)a / 255.0|   (fp64 steps)      n = the number of valid pixels
 * out fp32 [4] on the device:
 *   out[0] = (float)(S1 / S2)   the alpha-weighted mean angular error in degrees; NaN when S2 == 0 (no valid pixel)
 *   out[1] = (float)(S2 / 255.0)   the weight behind it: the valid pixels' summed alpha
 *   out[2] = (float)(S3 / P)   the mean absolute alpha error; 0 when accumulation is NULL
 *   out[3] = (float)n   exact: P <= 2^24
 * A non-finite predicted row of a valid pixel gives that pixel a non-finite deg and so a non-finite out[0]: it is not masked.  A
 * non-finite accumulation makes out[2] non-finite.
 *
 * Launches: one lane per pixel in a grid-stride loop, G = min(ceil(P / 256), RSN_NORMAL_ERROR_MAX_GROUPS) workgroups of 256 lanes,
 * so the first P at which a lane takes a second pixel is 256*RSN_NORMAL_ERROR_MAX_GROUPS + 1.  A lane adds its pixels in ascending
 * order; the 64 lanes of a wave are added by a butterfly (offsets 32, 16, ... 1), the four waves of a workgroup in order, and the
 * workgroup stores one record of four doubles (S1, S2, S3, n) at workspace[32 * group].  A second launch of one workgroup adds the
 * G records the same way (lane i holds record i) and writes out.  No atomics: two runs give the same bits of out and error_map,
 * and out does not depend on whether error_map is given.  workspace: device memory of at least rsn_normal_error_workspace_bytes
 * bytes (32 G; 0 for a P outside the limits), 8-byte aligned, contents irrelevant.  No allocation, no synchronisation, no
 * device-to-host read.
 * RSN_ERR_INVALID_ARGUMENT before any launch, with the reason in rsn_last_error(): n_pixels <= 0 or n_pixels > 2^24
 * (RSN_NORMAL_ERROR_MAX_PIXELS); a NULL normals, gt_normals, gt_rgba, workspace or out; a workspace that is not 8-byte aligned.
 * RSN_ERR_WORKSPACE for a workspace_bytes below the size needed. */
#define RSN_NORMAL_ERROR_MAX_GROUPS 256
#define RSN_NORMAL_ERROR_MAX_PIXELS (1 << 24)
size_t rsn_normal_error_workspace_bytes(int32_t n_pixels);
int rsn_normal_error(int32_t n_pixels, const float* normals, const float* accumulation, const uint8_t* gt_normals,
                     const uint8_t* gt_rgba, const float* rotation, float* error_map, void* workspace, size_t workspace_bytes,
                     float* out, void* stream);


/* ---- depth supervision (additive to ABI 18: no existing call changes): a capture's depth maps as a training target (the DS-NeRF
 * term) and as an eval metric.  A target is a distance along the NORMALISED ray, in scene units; 0 means "no target".
 *
 * rsn_gather_ray_depth: t [R] of the rays a sampler drew.  One lane per ray, one launch, no atomics, no host read.
 *   indices int32 [R,3] = (image, y, x) as the samplers write them; level int32 [R] or NULL (rsn_sample_pyramid_rays' output);
 *   depths fp32 [N,H,W], 0 = no measurement; cameras: the level-0 camera table fp32 [N, camera_stride] (9 or 12 columns,
 *   "captures") or NULL, in which case the four shared intrinsics fx .. cy are read instead (they are not read otherwise).
 *   t[r] = 0 when the stored depth is 0, when level[r] > 0 (the pyramid builds no depth levels: multi-scale training supervises
 *   only its level-0 rays -- a design rule, not a limit of the kernel), or when an index lies outside [N,H,W].
 *   euclidean != 0: the files hold distances along the ray, t[r] = the stored value.
 *   euclidean == 0 (the default of the loader: Polycam and Record3D write z-depths): t[r] = (float)((double)z * |v|), with
 *   v = (X, -Y, -1) the un-normalised camera-space direction of the pixel centre in fp64: (X, Y) = ((x+.5-cx)/fx, (y+.5-cy)/fy) for
 *   a row whose five coefficients are zero, and the Newton solve of "captures" (10 iterations, fp64) from that point otherwise.
 *   A fisheye row has a unit v and no z-plane beyond 90 degrees: the caller states whether the table holds one (has_fisheye; the
 *   table is on the device and is not read by the host), and has_fisheye != 0 with euclidean == 0 is RSN_ERR_INVALID_ARGUMENT
 *   before any launch.  (A fisheye row met by the kernel with euclidean == 0 gives 0.)
 *   RSN_ERR_INVALID_ARGUMENT before any launch also for: n_images, height or width < 1, n_rays < 0, a camera_stride other than 9 or
 *   12 with a table, has_fisheye with a 9-column table or none, fx or fy == 0 without a table, and, with n_rays > 0, a NULL
 *   indices, depths or t.  n_rays == 0 launches nothing. */
int rsn_gather_ray_depth(int32_t n_rays, const int32_t* indices, const int32_t* level, const float* depths, int32_t n_images,
                         int32_t height, int32_t width, const float* cameras, int32_t camera_stride, float fx, float fy, float cx,
                         float cy, int32_t has_fisheye, int32_t euclidean, float* t, void* stream);

/* The DS-NeRF depth term (Deng et al. 2022; nerfstudio's ds_nerf_depth_loss) of one primary level.  Per ray, with the target
 * D = target[r], the euclidean bins e_0 <= ... <= e_S (euclid_bins [R,S+1]), midpoints m_k = (e_k + e_{k+1}) / 2, lengths
 * l_k = e_{k+1} - e_k, the compositing weights w_k and s = depth_sigma, a standard deviation in scene units:
 *   L_ray        = [D > 0] sum_k -log(w_k + EPS) exp(-(m_k - D)^2 / (2 s^2)) l_k                      EPS = 1e-7
 *   dL_ray/dw_k  = -[D > 0] exp(-(m_k - D)^2 / (2 s^2)) l_k / (w_k + EPS)
 * This formula is the definition.  (nerfstudio's version is remembered to divide by 2 sigma, which would make its
 * depth_sigma = 0.01 an s of 0.1 here; that was not checked against its source.)
 * Both calls take sigma [R,S] and euclid_bins, the inputs of the level's rsn_composite call, not its fp32 weights: they form
 * w_k = -expm1(-x_k) exp(-X_k), x_k = l_k sigma_k, X_k = sum_{j<k} x_j in fp64, as rsn_distortion_backward does.  rsn_composite's
 * weights are good to 2^-24 of the transmittance and EPS is 2^-23: log(w + EPS) and 1 / (w + EPS) of a thin sample -- a target in
 * what is still empty space, the state the term acts on most -- would be off by tens of percent.  The interior is fp64 and the
 * result is rounded to fp32 once.
 * One wave per ray, 64-sample chunks with a carried scan, no atomics, a fixed order of addition: the same inputs give the same bits.
 * n_dev (or NULL): device-side ray count, min(n_rays, *n_dev) rows are processed and the rows behind are not touched.
 *
 * rsn_depth_loss_forward: loss_ray [R] = L_ray, unscaled; exactly 0 for a ray without a target.
 * rsn_depth_loss_backward: g_w[k] = g_loss_ray[r] dL_ray/dw_k is recomputed (nothing [R,S]-sized is kept from the forward) and
 *   carried to sigma by rsn_composite_backward's rule, g_sigma[k] = l_k (g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i), the suffix sum
 *   added up from the far end of the ray.  accumulate != 0: the value, rounded to fp32, is ADDED to g_sigma [R,S] (a ray without a
 *   target is left as it is); 0: it overwrites (zeros for such a ray).
 *
 * Before any launch: RSN_ERR_INVALID_ARGUMENT for n_rays < 0, n_samples < 1, a depth_sigma that is not a positive finite number
 * or, with n_rays > 0, a NULL pointer other than n_dev; RSN_ERR_UNSUPPORTED for n_samples > 4096.  n_rays == 0 launches nothing. */
int rsn_depth_loss_forward(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* euclid_bins, const float* sigma,
                           const float* target, float depth_sigma, float* loss_ray, void* stream);
int rsn_depth_loss_backward(int32_t n_rays, const int32_t* n_dev, int32_t n_samples, const float* euclid_bins, const float* sigma,
                            const float* target, float depth_sigma, const float* g_loss_ray, float* g_sigma, int32_t accumulate,
                            void* stream);

/* rsn_depth_error: one eval view's rendered depth against its target distances (rsn_gather_ray_depth over the whole view).
 * depth, target fp32 [P]; mask uint8 [P] or NULL (a capture's mask: 0 = the pixel is not scored).  Over the pixels with
 * target > 0 and a live mask byte, in fp64 and in rsn_normal_error's fixed order (same launch shape, same workspace: at least
 * rsn_normal_error_workspace_bytes(n_pixels) bytes, 8-byte aligned), no atomics, no host read:
 *   out[0] = (float)sum |depth - target|    out[1] = (float)sum (depth - target)^2    out[2] = (float)count   (exact: P <= 2^24)
 * RSN_ERR_INVALID_ARGUMENT before any launch: n_pixels outside [1, 2^24], a NULL depth, target, workspace or out, a misaligned
 * workspace; RSN_ERR_WORKSPACE for a workspace_bytes below the size needed. */
int rsn_depth_error(int32_t n_pixels, const float* depth, const float* target, const uint8_t* mask, void* workspace,
                    size_t workspace_bytes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RSN_H */
