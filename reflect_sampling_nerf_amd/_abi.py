"""ctypes binding of include/rsn.h (librsn_hip.so).

There is NO fallback: if the library is missing or does not export the ABI of include/rsn.h the
import of the product path raises.  Tensors are passed as raw device pointers (`tensor.data_ptr()`),
the stream as `torch.cuda.current_stream().cuda_stream`; the library never allocates or synchronises.
"""
import ctypes as C
import os

import torch

from ._build import LIB_PATH

RSN_ABI_VERSION = 18
RSN_MAX_TRUNK_LAYERS = 16
RSN_NUM_FREQS = 16
RSN_SPACING_UNIFORM = 0
RSN_SPACING_RECIPROCAL = 1
RSN_MMA_F32, RSN_MMA_BF16X6, RSN_MMA_BF16X3, RSN_MMA_BF16 = 0, 1, 2, 3
RSN_MMA_F32_FOLDED = 4  # exact fp32 training with field_output_bottleneck folded into mlp_mid (a descriptor value, not a Field mode)
RSN_VIS_RGB, RSN_VIS_UNIT, RSN_VIS_GRAY, RSN_VIS_LUT = 0, 1, 2, 3
RSN_NORMAL_ERROR_MAX_GROUPS = 256  # workgroups of 256 lanes: rsn_normal_error takes a second trip of its loop from 65,537 pixels on
RSN_NORMAL_ERROR_MAX_PIXELS = 1 << 24

_fp = C.c_void_p  # device float*


class FieldDesc(C.Structure):
    _fields_ = [
        ("num_layers", C.c_int32),
        ("width", C.c_int32),
        ("skip_layer", C.c_int32),
        ("mid_width", C.c_int32),
        ("density_bias", C.c_float),
        ("freqs", C.c_float * RSN_NUM_FREQS),
        ("mma_mode", C.c_int32),
        ("param_width", C.c_int32),
    ]


class FieldParams(C.Structure):
    _fields_ = [
        ("trunk_w", _fp * RSN_MAX_TRUNK_LAYERS),
        ("trunk_b", _fp * RSN_MAX_TRUNK_LAYERS),
        ("density_w", _fp), ("density_b", _fp),
        ("normals_w", _fp), ("normals_b", _fp),
        ("roughness_w", _fp), ("roughness_b", _fp),
        ("diff_w", _fp), ("diff_b", _fp),
        ("tint_w", _fp), ("tint_b", _fp),
        ("bottleneck_w", _fp), ("bottleneck_b", _fp),
        ("mid_w", _fp), ("mid_b", _fp),
        ("rgb_w", _fp), ("rgb_b", _fp),
    ]


class FieldOutputs(C.Structure):
    _fields_ = [(n, _fp) for n in
                ("sigma", "color", "pred_normals", "n_dot_d", "diff", "tint", "roughness", "raw_density",
                 "raw_roughness")]


class FieldSaved(C.Structure):
    _fields_ = [(n, _fp) for n in ("enc", "act", "bott", "sh", "hid", "heads", "normals", "relu_bits")]


class FieldJob(C.Structure):
    """rsn_field_job: one evaluation of a multi-evaluation training launch (rsn_field_forward_train_jobs)."""
    _fields_ = [("kind", C.c_int32), ("n_rays", C.c_int32), ("n_dev", C.c_void_p), ("n_samples", C.c_int32),
                ("origins", _fp), ("directions", _fp), ("pixel_area", _fp), ("euclid_bins", _fp), ("sqradius", _fp),
                ("out_rgb", _fp), ("out", C.POINTER(FieldOutputs)), ("saved", C.POINTER(FieldSaved))]


class FieldGradsIn(C.Structure):
    _fields_ = [(n, _fp) for n in ("sigma", "color", "pred_normals", "n_dot_d", "roughness", "ray_pn_loss", "ray_ori_loss",
                                   "weights")]


class FieldGradsOut(C.Structure):
    _fields_ = [(n, _fp) for n in ("dz_rgb", "da_mid", "d_bott", "dz_heads", "dy", "d_input")]


class FieldBwdJob(C.Structure):
    """rsn_field_bwd_job: one evaluation of a multi-evaluation backward launch (rsn_field_backward_jobs)."""
    _fields_ = [("kind", C.c_int32), ("n_rays", C.c_int32), ("n_dev", C.c_void_p), ("n_samples", C.c_int32),
                ("need_input_grad", C.c_int32), ("origins", _fp), ("directions", _fp), ("pixel_area", _fp),
                ("euclid_bins", _fp), ("sqradius", _fp), ("g_rgb", _fp), ("fwd", C.POINTER(FieldOutputs)),
                ("saved", C.POINTER(FieldSaved)), ("gin", C.POINTER(FieldGradsIn)), ("gout", C.POINTER(FieldGradsOut))]


class WGradJob(C.Structure):
    """rsn_wgrad_job: one reduction of a job-parallel weight-gradient launch (rsn_weight_grad_jobs)."""
    _fields_ = [("dy", C.POINTER(C.c_void_p)), ("x", C.POINTER(C.c_void_p)), ("col_map", C.c_void_p), ("dw", C.c_void_p),
                ("ld_dw", C.c_int32), ("db", C.c_void_p)]


class CompositeBwdIO(C.Structure):
    _fields_ = [(n, _fp) for n in ("sigma", "euclid_bins", "color", "bg_rgb", "roughness", "weights", "g_rgb",
                                   "g_roughness", "g_accumulation", "g_sigma", "g_color", "g_roughness_sample",
                                   "g_bg")]


class CompositeIO(C.Structure):
    _fields_ = [(n, _fp) for n in
                ("sigma", "euclid_bins", "color", "bg_rgb", "diff", "tint", "pred_normals", "roughness",
                 "weights", "rgb", "accumulation", "depth", "diff_out", "tint_out", "normals_out", "roughness_out",
                 "normals", "n_dot_d", "pn_loss_ray", "ori_loss_ray")]


class ReflectIO(C.Structure):
    _fields_ = [(n, _fp) for n in
                ("origins", "directions", "accumulation", "depth", "pred_normals", "roughness", "mask", "n_masked",
                 "ray_index", "n_dot_d", "origins2", "directions2", "sqradius", "pixel_area2", "nears2", "fars2",
                 "reflect_coarse", "reflect_fine", "workspace")]


RSN_GUARD_MAX_TENSORS = 48


class GuardStats(C.Structure):
    """rsn_guard_stats: what rsn_radam_step_guarded records on the device (train_ops.FusedRAdam.guard_stats reads it)."""
    _fields_ = [("last_norm", C.c_float), ("last_coef", C.c_float), ("last_skipped", C.c_int32), ("skipped_total", C.c_int32),
                ("last_skipped_step", C.c_int32), ("reserved", C.c_int32),
                ("per_tensor_sq", C.c_double * RSN_GUARD_MAX_TENSORS),
                ("per_tensor_sq_at_last_skip", C.c_double * RSN_GUARD_MAX_TENSORS)]


_SIGNATURES = {
    "rsn_abi_version": (C.c_int, []),
    "rsn_last_error": (C.c_char_p, []),
    "rsn_packed_weights_bytes": (C.c_size_t, [C.POINTER(FieldDesc)]),
    "rsn_pack_weights": (C.c_int, [C.POINTER(FieldDesc), C.POINTER(FieldParams), _fp, C.c_size_t, C.c_void_p]),
    "rsn_pack_table_bytes": (C.c_size_t, []),
    "rsn_pack_weights_table": (C.c_int, [C.POINTER(FieldDesc), C.POINTER(FieldParams), _fp, C.c_size_t, _fp, C.c_size_t,
                                         C.c_int32, C.c_void_p]),
    "rsn_sample_spaced": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_float, _fp, _fp, _fp, _fp, _fp,
                                    C.c_void_p]),
    "rsn_sample_pdf": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _fp, _fp,
                                 _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_field_forward_frustum": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp,
                                            _fp, C.POINTER(FieldOutputs), C.c_void_p]),
    "rsn_field_forward_frustum_train": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, C.c_int32, _fp, _fp,
                                                  _fp, _fp, C.POINTER(FieldOutputs), C.POINTER(FieldSaved),
                                                  C.c_void_p]),
    "rsn_field_backward_frustum": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, _fp,
                                             C.POINTER(FieldOutputs), C.POINTER(FieldSaved),
                                             C.POINTER(FieldGradsIn), C.POINTER(FieldGradsOut), C.c_int32,
                                             C.c_void_p]),
    "rsn_field_forward_inf_train": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp, _fp,
                                              C.POINTER(FieldSaved), C.c_void_p]),
    "rsn_field_backward_inf": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp, C.POINTER(FieldSaved),
                                         _fp, C.POINTER(FieldGradsOut), C.c_int32, C.c_void_p]),
    "rsn_composite_backward": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(CompositeBwdIO), C.c_void_p]),
    "rsn_distortion_forward": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, C.c_void_p]),
    "rsn_distortion_backward": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, _fp, _fp, C.c_int32, C.c_void_p]),
    "rsn_weight_grad": (C.c_int, [C.c_int64, _fp, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, C.c_int32,
                                  _fp, C.c_void_p]),
    "rsn_sh34_encode": (C.c_int, [C.c_int64, _fp, _fp, _fp, C.c_void_p]),
    "rsn_ipe_encode": (C.c_int, [C.c_int64, _fp, _fp, C.POINTER(C.c_float), _fp, C.c_void_p]),
    "rsn_weight_grad_multi": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int32, C.c_int32,
                                        C.POINTER(C.c_void_p), C.c_int32, C.c_int32, _fp, C.c_void_p, C.c_int32, _fp,
                                        C.c_void_p]),
    "rsn_weight_grad_multi_mode": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int32, C.c_int32,
                                             C.POINTER(C.c_void_p), C.c_int32, C.c_int32, _fp, C.c_void_p, C.c_int32, _fp,
                                             C.c_int32, C.c_void_p]),
    "rsn_field_forward_train_jobs": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, C.POINTER(FieldJob), C.c_void_p]),
    "rsn_field_backward_jobs": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, C.POINTER(FieldBwdJob), C.c_void_p]),
    "rsn_weight_grad_multi_dev": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32,
                                            C.c_int32, _fp, C.c_void_p, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_void_p]),
    "rsn_weight_grad_jobs": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32,
                                       C.POINTER(WGradJob), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p]),
    "rsn_weight_grad_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_int32]),
    "rsn_weight_grad_multi_dev_ordered": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32,
                                                    C.c_int32, _fp, C.c_void_p, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_void_p,
                                                    C.c_size_t, C.c_void_p]),
    "rsn_weight_grad_jobs_ordered": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                               C.c_int32, C.POINTER(WGradJob), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rsn_unfold_bottleneck_grads": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp, _fp, _fp,
                                              C.c_void_p]),
    "rsn_loss_forward_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, C.POINTER(_fp), C.POINTER(_fp),
                                            C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_float), _fp,
                                            C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.c_void_p]),
    "rsn_loss_rays_forward": (C.c_int, [C.c_int32, _fp, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_float),
                                        _fp, C.POINTER(_fp), C.c_void_p]),
    "rsn_loss_rays_backward": (C.c_int, [C.c_int32, _fp, C.POINTER(C.c_float), C.POINTER(_fp), C.POINTER(_fp),
                                         C.POINTER(_fp), C.c_void_p]),
    "rsn_loss_scale_grads": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp),
                                       C.c_void_p]),
    "rsn_radam_step": (C.c_int, [C.c_int32, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp),
                                 C.POINTER(C.c_int32), C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_void_p]),
    "rsn_grad_sumsq_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(C.c_int32)]),
    "rsn_grad_sumsq": (C.c_int, [C.c_int32, C.POINTER(_fp), C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "rsn_radam_step_guarded": (C.c_int, [C.c_int32, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp),
                                         C.POINTER(C.c_int32), C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rsn_colsum": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_void_p]),
    "rsn_ray_sum": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_void_p]),
    "rsn_reflect_backward": (C.c_int, [C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_reflect_default_backward": (C.c_int, [C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_reflect_combine_backward": (C.c_int, [C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_field_forward_inf": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_field_forward_embedding": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp,
                                              C.POINTER(FieldOutputs), C.c_void_p]),
    "rsn_gaussians": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_contract": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_reflection": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_field_forward_gaussians": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp,
                                              C.POINTER(FieldOutputs), _fp, C.c_void_p]),
    "rsn_field_forward_gaussians_train": (C.c_int, [C.POINTER(FieldDesc), _fp, C.c_int32, _fp, _fp, _fp,
                                                    C.POINTER(FieldOutputs), _fp, C.POINTER(FieldSaved), C.c_void_p]),
    "rsn_composite": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(CompositeIO),
                                C.c_void_p]),
    "rsn_reflect_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "rsn_reflect_setup": (C.c_int, [C.c_int32, C.c_float, C.POINTER(ReflectIO), C.c_void_p]),
    "rsn_reflect_combine": (C.c_int, [C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_train_saved_layout": (C.c_int, [C.POINTER(FieldDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rsn_sample_camera_rays": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _fp, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _fp, _fp, _fp, _fp,
                                         C.c_void_p, C.c_void_p]),
    "rsn_camera_rays_image": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_float, C.c_float, C.c_float, C.c_float, _fp, _fp, _fp,
                                        C.c_void_p]),
    "rsn_build_pyramid": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _fp, C.c_size_t, C.c_void_p]),
    "rsn_sample_pyramid_rays": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _fp, C.c_size_t, _fp, C.c_float,
                                          C.c_float, C.c_float, C.c_float, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _fp, _fp,
                                          _fp, _fp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rsn_sample_capture_rays": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _fp, C.c_size_t, _fp, _fp,
                                          C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rsn_capture_rays_image": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "rsn_live_pixels_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rsn_build_live_pixels": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "rsn_sample_capture_rays_live": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _fp, C.c_size_t, _fp, _fp,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _fp,
                                               _fp, _fp, _fp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rsn_capture_rays_image2": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp, C.c_void_p]),
    "rsn_ssim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rsn_ssim": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_void_p, C.c_size_t, _fp, C.c_void_p]),
    "rsn_mesh_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rsn_mesh_count": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rsn_mesh_emit": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, _fp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rsn_tsdf_integrate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, _fp,
                                     C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _fp, C.c_float, C.c_float,
                                     _fp, _fp, C.c_void_p]),
    "rsn_visualize": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_float, C.c_float, _fp, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p]),
    "rsn_occupancy_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rsn_occupancy_build": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rsn_occupancy_cull_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "rsn_occupancy_cull": (C.c_int, [C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "rsn_scatter_rows": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, _fp, C.c_int32, C.c_float, _fp, C.c_void_p]),
    "rsn_occupancy_samples_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rsn_occupancy_compact_samples": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32,
                                                C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int32, C.c_float,
                                                C.c_void_p, C.c_void_p, C.c_void_p, _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p]),
    "rsn_scatter_level": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(FieldOutputs), C.POINTER(FieldOutputs), C.c_void_p]),
    "rsn_pointcloud_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rsn_pointcloud_mark": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _fp, _fp,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "rsn_pointcloud_select": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _fp, _fp,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                        _fp, C.c_void_p]),
    "rsn_decimate_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rsn_decimate_cluster": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rsn_decimate_resolve": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_void_p]),
    "rsn_decimate_count": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p]),
    "rsn_decimate_emit": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, _fp, C.c_void_p, C.c_void_p]),
    "rsn_texture_points": (C.c_int, [C.c_int32, _fp, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, _fp, _fp, C.c_void_p]),
    "rsn_normal_error_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "rsn_normal_error": (C.c_int, [C.c_int32, _fp, _fp, C.c_void_p, C.c_void_p, _fp, _fp, C.c_void_p, C.c_size_t, _fp, C.c_void_p]),
    "rsn_gather_ray_depth": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32,
                                       C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, _fp, C.c_void_p]),
    "rsn_depth_loss_forward": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, C.c_float, _fp, C.c_void_p]),
    "rsn_depth_loss_backward": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, C.c_float, _fp, _fp, C.c_int32, C.c_void_p]),
    "rsn_depth_error": (C.c_int, [C.c_int32, _fp, _fp, C.c_void_p, C.c_void_p, C.c_size_t, _fp, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class RsnError(RuntimeError):
    pass


_lib = None


def load_library(path: str = LIB_PATH):
    """Load librsn_hip.so and bind every symbol of include/rsn.h.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RSN_LIBRARY", path)  # tools/: another build of the same ABI, e.g. from another checkout (A/B runs)
    if not os.path.exists(path):
        raise RsnError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or reflect_sampling_nerf_amd/_build.py). There is no CPU/eager fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RsnError(f"{path} does not export {name} (include/rsn.h)") from e
        fn.restype = res
        fn.argtypes = args
    ver = lib.rsn_abi_version()
    if ver != RSN_ABI_VERSION:
        raise RsnError(f"ABI version mismatch: library {ver}, binding {RSN_ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load_library().rsn_last_error()
        raise RsnError(f"librsn_hip error {rc}: {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def float3(v):
    """Three numbers -> the float[3] an origin or a spacing is passed as."""
    return (C.c_float * 3)(*[float(x) for x in v])


def check_f32_cuda(who: str, **tensors) -> None:
    """RsnError naming the first of `tensors` (None is skipped) that is not a contiguous fp32 tensor on a cuda (ROCm) device."""
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or t.device.type != "cuda" or not t.is_contiguous()):
            raise RsnError(f"{who}: {name} must be a contiguous fp32 tensor on a cuda (ROCm) device")
