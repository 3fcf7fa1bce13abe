"""ctypes binding of libngp_hip.so (include/ngp_hip.h).

This is the only place the package touches native code.  There is NO fallback:
if the shared library is missing or a call fails, a RuntimeError is raised --
the operators never route through PyTorch eager code or a CPU implementation.

The package enters the library through call() and sizes scratch with workspace(); lib, check, ptr and stream are
what those are built from (tests, bench.py and scripts/ use them directly).

torch must be imported before the library is loaded so that both resolve the
same HIP runtime (libamdhip64.so.7) inside the process.
"""
import ctypes as C
import os

import torch  # noqa: F401  (loads the HIP runtime the library shares)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("NGP_HIP_LIB", os.path.join(_HERE, "libngp_hip.so"))   # (the override: A/B builds of experiments, scripts/build_variant.sh)

NGP_F32, NGP_F16 = 0, 1
NGP_PREC_F16, NGP_PREC_F32, NGP_PREC_F16_REF = 0, 1, 2          # ngp_model::precision
# enum ngp_debug_flag: the flag word of ngp_debug_disable_march_queue / ngp_render_ctx_set_debug (each bit switches one device off)
NGP_DBG_NO_BLOCK_JUMP, NGP_DBG_NO_COARSE, NGP_DBG_NO_SLOW_SORT, NGP_DBG_NO_LIN = 1 << 0, 1 << 1, 1 << 2, 1 << 3
NGP_DBG_ONE_ITER_PER_LAUNCH, NGP_DBG_NO_TILES = 1 << 8, 1 << 13
NGP_DBG_NO_PRE_VERDICT, NGP_DBG_WIDE_ITEMS, NGP_DBG_REPLAY_ONE_ITER = 1 << 14, 1 << 15, 1 << 16
NGP_DBG_LANE_MARCH, NGP_DBG_PROBE_PER_SAMPLE = 1 << 17, 1 << 18
NGP_SCHED_NO_FORECAST = 1                                        # ngp_render_ctx_set_schedule_flags (a context's own word, not the debug flag word)
NGP_EDT_INF = 0x7FFFFFFF                                         # ngp_edt_sq: no occupied cell
NGP_COMPONENTS_TILE = (4, 4, 16)                                 # NGP_COMPONENTS_TILE_X / _Y / _Z: the tile ngp_label_components labels in LDS

ABI_VERSION = 104                                               # NGP_ABI_VERSION of the header this table mirrors; lib() compares

_vp, _u32, _f32, _int, _sz = C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_size_t


class StreamPtr(C.c_void_p):
    """ngp_stream_t: the slot that call() fills with the current stream (to ctypes, a c_void_p like any other)"""


_st = StreamPtr


class ModelStruct(C.Structure):
    """struct ngp_model (include/ngp_hip.h)"""
    _fields_ = [
        ("embeddings", _vp), ("offsets_host", _vp), ("L", _u32), ("S", _f32), ("H_base", _u32), ("gridtype", _u32),
        ("align_corners", _int), ("sigma_weights", _vp), ("sigma_hidden_mm", _u32), ("color_weights", _vp),
        ("color_hidden_mm", _u32), ("bound", _f32), ("density_scale", _f32), ("density_bitfield", _vp),
        ("cascade", _u32), ("grid_size", _u32), ("cell_tables", _vp), ("cell_levels", _u32), ("packed_weights", _vp),
        ("precision", _u32),
    ]


class RenderStats(C.Structure):
    """struct ngp_render_stats"""
    _fields_ = [("samples_marched", C.c_uint64), ("samples_slots", C.c_uint64), ("iterations", _u32), ("rays", _u32),
                ("last_n_alive", _u32), ("last_n_step", _u32), ("launches", _u32), ("replayed", _u32)]


class RaycastGrid(C.Structure):
    """struct ngp_raycast_grid"""
    _fields_ = [("lo", _f32 * 3), ("cell", _f32 * 3), ("inv_cell", _f32 * 3), ("grow", _f32 * 3), ("reach", _f32), ("n", _u32 * 3)]


class VoxelBox(C.Structure):
    """struct ngp_voxel_box"""
    _fields_ = [("start", C.c_double * 3), ("granularity", C.c_double), ("shape", _u32 * 3), ("axis", C.c_int32 * 3), ("sign", C.c_int32 * 3)]


# name -> argtypes (restype is int unless listed in _RESTYPES).  Mirrors include/ngp_hip.h one to one, _st where the header says
# ngp_stream_t; tests/test_abi.py compares every entry with its prototype (count, kind and width of each parameter, return type).
SIGNATURES = {
    "ngp_last_error": [],
    "ngp_version": [],
    "ngp_device_count": [],
    "ngp_finish_rays": [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_float), _u32, _st],
    "ngp_near_far_from_aabb": [_vp, _vp, _vp, _u32, _f32, _vp, _vp, _st],
    "ngp_sph_from_ray": [_vp, _vp, _f32, _u32, _vp, _st],
    "ngp_morton3D": [_vp, _u32, _vp, _st],
    "ngp_morton3D_invert": [_vp, _u32, _vp, _st],
    "ngp_packbits": [_vp, _u32, _f32, _vp, _st],
    "ngp_march_rays_train_workspace": [_u32],
    "ngp_march_rays_train": [_vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                             _u32, _vp, _sz, _st],
    "ngp_composite_rays_train_forward": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _st],
    "ngp_composite_rays_train_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _st],
    "ngp_march_rays": [_u32, _u32, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32,
                       _u32, _st],
    "ngp_occupancy_lin_bytes": [_u32, _u32],
    "ngp_build_occupancy_lin": [_vp, _u32, _u32, _vp, _sz, _st],
    "ngp_march_rays_lin": [_u32, _u32, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32,
                           _u32, _vp, _st],
    "ngp_composite_rays": [_u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _st],
    "ngp_grid_encode_forward": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _u32, _int, _int, _vp, _u32, _st],
    "ngp_grid_encode_backward": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _vp, _u32, _int,
                                 _int, _vp, _sz, _st],
    "ngp_grid_encode_forward_strided": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _u32, _int, _int, _vp, _u32,
                                        _u32, _u32, _st],
    "ngp_grid_encode_backward_strided": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _vp, _u32, _int,
                                         _int, _vp, _sz, _u32, _u32, _st],
    "ngp_grid_encode_backward_workspace": [_u32, _u32, _u32, _u32, _int],
    "ngp_sh_encode_forward": [_vp, _vp, _u32, _u32, _u32, _int, _vp, _st],
    "ngp_sh_encode_backward": [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_freq_encode_forward": [_vp, _vp, _u32, _u32, _u32, _st],
    "ngp_freq_encode_backward": [_vp, _vp, _u32, _u32, _u32, _vp, _st],
    "ngp_ff_sigma_color_input": [_vp, _vp, _u32, _u32, _vp, _vp, _st],
    "ngp_ff_sigma_color_input_backward": [_vp, _vp, _vp, _u32, _u32, _vp, _st],
    "ngp_ff_rgb": [_vp, _u32, _vp, _st],
    "ngp_ff_rgb_backward": [_vp, _vp, _u32, _u32, _vp, _st],
    "ngp_ffmlp_forward": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_ffmlp_inference": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_ffmlp_backward": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _int, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_ffmlp_forward_planes": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_ffmlp_backward_planes": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _int, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_ffmlp_backward_recomputes": [_u32, _u32, _u32],
    "ngp_ffmlp_backward_workspace": [_u32, _u32, _u32, _u32],
    "ngp_ffmlp_backward_buffer_bytes": [_u32, _u32, _u32, _u32],
    "ngp_ffmlp_allocate_splitk": [_sz],
    "ngp_ffmlp_free_splitk": [],
    "ngp_get_rays": [_vp, _u32, _f32, _f32, _f32, _f32, _u32, _u32, _vp, _u32, _vp, _vp, _st],
    "ngp_get_rays_backward": [_vp, _vp, _u32, _f32, _f32, _f32, _f32, _u32, _u32, _vp, _u32, _vp, _st],
    "ngp_uq_stats_workspace": [],
    "ngp_uq_stats": [_vp, _int, _vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp, _sz, _st],
    "ngp_sigma_fit_workspace": [_u32, _u32],
    "ngp_sigma_fit_eval": [_vp, _vp, _u32, _vp, _f32, C.c_double, _int, _u32, _vp, _sz, _vp, _vp, _st],
    "ngp_sigma_fit_step": [_vp, _vp, _u32, _vp, _f32, C.c_double, _int, _u32, _vp, _sz, _vp, _vp, _vp, _f32, _u32, _vp, _vp, _vp, _u32, _st],
    "ngp_adam_step": [_vp, _vp, _vp, _vp, C.c_uint64, _f32, _f32, _f32, _f32, _u32, _f32, _st],
    "ngp_adam_advance_step": [_vp, _vp, _st],
    "ngp_adam_step_dev": [_vp, _vp, _vp, _vp, C.c_uint64, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _st],
    "ngp_train_targets": [_vp, _int, _u32, C.c_uint64, _u32, _vp, _u32, _vp, _vp, _int, _vp, _st],
    "ngp_train_depth_targets": [_vp, C.c_uint64, _u32, _u32, _vp, _u32, _f32, _f32, _f32, _f32, _f32, _vp, _st],
    "ngp_photo_loss_workspace": [_u32],
    "ngp_photo_loss_forward": [_vp, _int, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _sz, _st],
    "ngp_photo_loss_backward": [_vp, _int, _vp, _u32, _vp, _vp, _st],
    "ngp_distortion_workspace": [_u32],
    "ngp_distortion_train_forward": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_distortion_train_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _st],
    "ngp_distortion_forward": [_vp, _vp, _vp, _f32, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_distortion_backward": [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _u32, _u32, _vp, _st],
    "ngp_depth_loss_workspace": [_u32],
    "ngp_depth_loss_train_forward": [_vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_depth_loss_train_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _u32, _u32, _vp, _st],
    "ngp_depth_loss_forward": [_vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_depth_loss_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _u32, _u32, _vp, _st],
    "ngp_image_quality_workspace": [_u32, _u32, _u32],
    "ngp_image_quality": [_vp, _vp, _vp, _u32, _u32, _u32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _f32, _vp, _vp, _vp, _sz, _st],
    "ngp_cell_tables_bytes": [C.POINTER(ModelStruct), _u32],
    "ngp_build_cell_tables": [C.POINTER(ModelStruct), _u32, _vp, _st],
    "ngp_packed_weights_bytes": [],
    "ngp_pack_weights": [C.POINTER(ModelStruct), _vp, _st],
    "ngp_render_ctx_create": [_u32, C.POINTER(_vp)],
    "ngp_render_ctx_destroy": [_vp],
    "ngp_render_ctx_set_frame_width": [_vp, _u32],
    "ngp_render_ctx_set_schedule_flags": [_vp, _u32],
    "ngp_render_ctx_schedule_stats": [_vp, C.POINTER(C.c_uint64)],
    "ngp_render_rays": [_vp, C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _u32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _vp,
                        C.POINTER(C.c_float), C.POINTER(RenderStats), _int, _st],
    "ngp_network_forward": [C.POINTER(ModelStruct), _vp, _vp, _u32, _vp, _vp, _st],
    "ngp_network_density": [C.POINTER(ModelStruct), _vp, _u32, _vp, _vp, _st],
    "ngp_network_density_backward": [C.POINTER(ModelStruct), _vp, _vp, _u32, _vp, _vp, _vp, _st],
    "ngp_planner_collision": [C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _u32, _u32, _vp, _st],
    "ngp_planner_collision_backward": [C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _st],
    "ngp_cell_max_density": [C.POINTER(ModelStruct), _vp, C.c_float, _u32, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_edt_sq_workspace": [_u32, _u32, _u32],
    "ngp_edt_sq": [_vp, _u32, _u32, _u32, _vp, _vp, _sz, _st],
    "ngp_label_components_workspace": [_u32, _u32, _u32],
    "ngp_label_components": [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _sz, _st],
    "ngp_component_stats": [_vp, _u32, _u32, _u32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _st],
    "ngp_isosurface_workspace": [_u32, _u32, _u32],
    "ngp_isosurface_count": [_vp, _u32, _u32, _u32, _f32, _vp, _sz, _vp, _st],
    "ngp_isosurface_emit": [_vp, _u32, _u32, _u32, _f32, _vp, _sz, C.c_uint64, C.c_uint64, _vp, _vp, _st],
    "ngp_simplify_keys": [_vp, _u32, _vp, _u32, C.POINTER(C.c_double), C.c_double, _vp, _vp, _st],
    "ngp_simplify_corners": [_vp, _u32, _u32, _vp, _vp, _st],
    "ngp_simplify_accumulate": [_vp, _u32, _vp, _u32, C.POINTER(C.c_double), C.c_double, _int, _vp, _vp, _vp, _vp, _vp, _vp, _st],
    "ngp_simplify_faces": [_vp, _u32, _u32, _vp, _vp, _st],
    "ngp_simplify_emit": [_u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _st],
    "ngp_raycast_bin_count": [_vp, _u32, C.POINTER(RaycastGrid), _vp, _st],
    "ngp_raycast_bin_emit": [_vp, _u32, C.POINTER(RaycastGrid), _vp, C.c_uint64, _vp, _vp, _st],
    "ngp_raycast": [_vp, _vp, C.c_uint64, C.POINTER(RaycastGrid), _vp, _vp, C.c_uint64, _vp, _u32, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _st],
    "ngp_raycast_shade": [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _u32, _vp, _u32, _f32, C.POINTER(C.c_float), _vp, _vp, _st],
    "ngp_voxelize_count": [_vp, _u32, _vp, _u32, C.POINTER(VoxelBox), _vp, _vp, _st],
    "ngp_voxelize_mark": [_vp, _u32, _vp, _u32, C.POINTER(VoxelBox), _vp, C.c_uint64, C.c_uint64, _vp, _st],
    "ngp_box_mesh_overlap": [_vp, C.c_uint64, C.POINTER(RaycastGrid), _vp, _vp, C.c_uint64, _vp, _u32, _vp, _vp, _vp, _st],
    "ngp_box_cells_overlap": [_vp, C.POINTER(VoxelBox), _vp, C.c_uint64, _vp, _st],
    "ngp_box_mesh_clearance": [_vp, C.c_uint64, C.POINTER(RaycastGrid), _vp, _vp, C.c_uint64, _vp, _u32, _vp, _vp, C.c_double, _vp, _vp, _vp, _st],
    "ngp_box_cells_clearance": [_vp, C.POINTER(VoxelBox), _vp, C.c_uint64, C.c_double, _vp, _vp, _vp, _st],
    "ngp_overlay_cast": [_vp, _vp, C.c_uint64, _vp, _vp, _u32, _f32, _vp, _u32, _vp, _vp, _vp, _st],
    "ngp_overlay_shade": [_vp, _vp, _vp, C.c_uint64, _vp, _u32, _f32, _vp, _vp, _st],
    "ngp_closest_point": [_vp, C.c_uint64, C.POINTER(RaycastGrid), _vp, _vp, C.c_uint64, _vp, _u32, _f32, _vp, _vp, _vp, _vp, _st],
    "ngp_distance_stats_state_bytes": [],
    "ngp_distance_stats_workspace": [C.c_uint64],
    "ngp_distance_stats": [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_float), _u32, _vp, _vp, _vp, _sz, _st],
    "ngp_sift_workspace": [_u32, _u32],
    "ngp_sift_layer_offset": [_u32, _u32, _int, _int],
    "ngp_sift_octaves": [_u32, _u32],
    "ngp_sift_interest_mask": [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _st],
    "ngp_render_uniform_backward_lds": [C.POINTER(ModelStruct), _u32],
    "ngp_packed_weights_bwd_bytes": [],
    "ngp_pack_weights_bwd": [C.POINTER(ModelStruct), _vp, _st],
    "ngp_render_uniform_backward": [C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _st],
    "ngp_uniform_samples": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(C.c_float), _vp, _vp, _st],
    "ngp_uniform_samples_backward": [_vp, _vp, _vp, _vp, _u32, _u32, C.POINTER(C.c_float), _vp, _vp, _st],
    "ngp_transmittance_weights": [_vp, _vp, _vp, _u32, _u32, _f32, _vp, _st],
    "ngp_transmittance_weights_backward": [_vp, _vp, _vp, _vp, _u32, _u32, _f32, _vp, _st],
    "ngp_sample_pdf": [_vp, _vp, _u32, _u32, _vp, _int, _u32, _vp, _st],
    "ngp_merge_sorted": [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _st],
    "ngp_mark_untrained_grid_workspace": [_u32, _u32, _u32],
    "ngp_mark_untrained_grid": [_vp, _u32, _f32, _f32, _f32, _f32, _f32, _u32, _u32, _vp, _vp, _sz, _st],
    "ngp_density_grid_points": [_vp, _u32, _u32, _f32, _vp, _vp, _vp, _st],
    "ngp_density_grid_workspace": [_u32, _u32],
    "ngp_density_grid_update": [_vp, _u32, _u32, _u32, _vp, _vp, _u32, _f32, _f32, _vp, _sz, _st],
    "ngp_density_grid_finish": [_vp, _u32, _u32, _f32, _vp, _vp, _vp, _sz, _st],
    "ngp_render_uniform": [C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _st],
    "ngp_render_upsample": [C.POINTER(ModelStruct), _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _sz, _st],
    "ngp_render_upsample_workspace": [_u32, _u32, _u32],
    "ngp_debug_set_stamps": [_vp],
    "ngp_debug_set_sample_hash": [_vp],
    "ngp_debug_disable_march_queue": [_int],
    "ngp_render_ctx_set_debug": [_vp, _int, _int, _vp, _vp],
    "ngp_debug_set_grad_dump": [_vp],
    "ngp_debug_fused_features": [C.POINTER(ModelStruct), _vp, _u32, _int, _vp, _st],
    "ngp_prof_enable": [_int],
    "ngp_prof_reset": [],
    "ngp_prof_read": [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)],
}
_RESTYPES = {"ngp_render_uniform_backward_lds": _sz, "ngp_cell_tables_bytes": _sz, "ngp_packed_weights_bytes": _sz, "ngp_packed_weights_bwd_bytes": _sz, "ngp_grid_encode_backward_workspace": _sz,
             "ngp_ffmlp_backward_workspace": _sz, "ngp_ffmlp_backward_buffer_bytes": _sz, "ngp_render_upsample_workspace": _sz, "ngp_density_grid_workspace": _sz, "ngp_mark_untrained_grid_workspace": _sz, "ngp_last_error": C.c_char_p, "ngp_march_rays_train_workspace": _sz, "ngp_uq_stats_workspace": _sz, "ngp_sigma_fit_workspace": _sz, "ngp_occupancy_lin_bytes": _sz, "ngp_edt_sq_workspace": _sz, "ngp_label_components_workspace": _sz, "ngp_isosurface_workspace": _sz, "ngp_sift_workspace": _sz, "ngp_sift_layer_offset": _sz, "ngp_photo_loss_workspace": _sz, "ngp_image_quality_workspace": _sz, "ngp_distortion_workspace": _sz, "ngp_depth_loss_workspace": _sz, "ngp_distance_stats_state_bytes": _sz, "ngp_distance_stats_workspace": _sz}

_lib = None


def lib():
    """Load libngp_hip.so (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no fallback implementation.")
        handle = C.CDLL(SO_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch: fail loudly
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
        if handle.ngp_version() != ABI_VERSION:
            raise RuntimeError(f"{SO_PATH} has ABI version {handle.ngp_version()}, this package binds version {ABI_VERSION}: "
                               "rebuild the library from this tree")
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().ngp_last_error()
        raise RuntimeError(f"libngp_hip {what} failed (code {rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """device pointer of a contiguous CUDA(HIP) tensor; None -> NULL"""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libngp_hip operators need tensors on a HIP device; got a CPU tensor (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("libngp_hip operators need contiguous tensors")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """torch's CURRENT stream of the current device (the reference launches on the legacy default stream).  Asked a dozen
    times per training step: the raw handle comes straight from torch's C layer when it offers it (a tenth of the cost of building a
    torch.cuda.Stream object each time)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_bound = {}      # name -> (ngp_{name}, its void* slots, its parameters without the stream, whether it takes one): made once per name
_current_stream, _Tensor, _bump = stream, torch.Tensor, torch.autograd.graph.increment_version


def _bind(name):
    argtypes = SIGNATURES.get("ngp_" + name)
    if argtypes is None:
        raise AttributeError(f"libngp_hip has no function ngp_{name}")
    takes_stream = bool(argtypes) and argtypes[-1] is StreamPtr
    bound = _bound[name] = ("ngp_" + name, tuple(i for i, t in enumerate(argtypes) if t is _vp), len(argtypes) - takes_stream, takes_stream)
    return bound


def call(name, *args, wrote=(), stream=None):
    """The one way into a status-returning function ngp_{name}: tensors become device pointers (ptr's rules), None is NULL, anything
    else passes as it is; the current stream (or `stream`, a raw handle) is appended when the function takes one; a non-zero
    status raises with ngp_last_error.  `wrote`: the tensors that outlive the caller and that the library writes through their
    pointers -- their version counters are bumped, which is what every cache of derived data in the package is keyed on."""
    symbol, pointer_slots, n, takes_stream = _bound.get(name) or _bind(name)
    fn = getattr(_lib or lib(), symbol)          # read from the handle on every call: tests wrap single entry points there
    if len(args) != n:
        raise TypeError(f"ngp_{name} takes {n} arguments{' and the stream' if takes_stream else ''}; {len(args)} given")
    argv = list(args)
    for i in pointer_slots:          # only a void* slot can take a tensor: the numbers between them cost nothing (a dozen calls per training step come through here)
        a = argv[i]
        if isinstance(a, _Tensor):   # ptr(a), its two conditions tested in place
            argv[i] = a.data_ptr() if a.is_cuda and a.is_contiguous() else ptr(a)
    if takes_stream:
        argv.append(_current_stream() if stream is None else stream)
    elif stream is not None:
        raise TypeError(f"ngp_{name} takes no stream")
    rc = fn(*argv)
    if rc:
        check(rc, name)
    if wrote:
        _bump(wrote)


def workspace(name, *dims, device):
    """(uint8 buffer or None, nbytes) of the size ngp_{name}_workspace(*dims) answers; None when that is 0."""
    nbytes = getattr(lib(), f"ngp_{name}_workspace")(*dims)
    return (torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None), nbytes


def dtype_code(t):
    if t.dtype == torch.float32:
        return NGP_F32
    if t.dtype == torch.float16:
        return NGP_F16
    raise RuntimeError(f"unsupported dtype {t.dtype}: the grid encoder supports float32 and float16")


def host_i32(t):
    """int32 host copy of a small device tensor (e.g. GridEncoder.offsets), cached ON the tensor object and keyed by its
    version counter.  (A cache keyed by data_ptr is wrong: the allocator hands a freed tensor's address to the next model.)"""
    cached = getattr(t, "_ngp_host_i32", None)
    if cached is not None and cached[0] == t._version and cached[1] == t.data_ptr():
        return cached[2]
    vals = t.detach().to("cpu", torch.int32).tolist()
    arr = (C.c_int32 * len(vals))(*vals)
    try:
        t._ngp_host_i32 = (t._version, t.data_ptr(), arr)
    except AttributeError:
        pass
    return arr
