"""ctypes binding of ``libsmilfit.so`` (C ABI: include/smilfit.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C smilify_amd/csrc``.  There is
NO fallback: if the shared object is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMILFIT_LIB: load another build of the same library (instrumented builds under tools/dbg); never a CPU path
LIB_PATH = os.environ.get("SMILFIT_LIB") or os.path.join(_HERE, "lib", "libsmilfit.so")

EXPORTS = [
    "smil_model_create", "smil_model_destroy", "smil_model_dims", "smil_last_error", "smil_version",
    "smil_lbs_forward", "smil_lbs_forward_project", "smil_lbs_backward", "smil_lbs_backward_ndc", "smil_lbs_backward_ndc_supported", "smil_clip_depth_backward", "smil_project", "smil_project2", "smil_project_backward", "smil_project_backward2",
    "smil_fov_reduce", "smil_fit_epilogue",
    "smil_raster_workspace_bytes", "smil_raster_stats", "smil_silhouette_forward", "smil_silhouette_backward",
    "smil_silhouette_l1_fused", "smil_prior_losses", "smil_mask_rows", "smil_joint_loss", "smil_pix_scale",
    "smil_image_abs_sum", "smil_sil_objective", "smil_window_terms", "smil_adam_step", "smil_adam_step_multi", "smil_adam_step_dev", "smil_profile_enable",
    "smil_profile_read", "smil_colour_workspace_bytes", "smil_render_colour",
    "smil_fragments_workspace_bytes", "smil_render_fragments", "smil_depth_visibility",
    "smil_sample_points", "smil_chamfer_workspace_bytes", "smil_chamfer", "smil_mesh_reg_workspace_bytes", "smil_mesh_regularisers",
    "smil_knn_workspace_bytes", "smil_knn", "smil_sdf_distance_workspace_bytes", "smil_sdf_distance", "smil_sample_vertices",
    "smil_sample_vertices_backward_workspace_bytes", "smil_sample_vertices_backward",
    "smil_ray_diameters_workspace_bytes", "smil_ray_diameters",
    "smil_fps", "smil_ball_query", "smil_group_points", "smil_group_points_backward_workspace_bytes", "smil_group_points_backward",
    "smil_triangulate",
    "smil_refine_workspace_bytes", "smil_refine_evaluate", "smil_refine_cameras",
    "smil_refine_points_evaluate", "smil_refine_points",
    "smil_image_bounds", "smil_warp_images",
    "smil_rot6d_to_matrix", "smil_rot6d_to_matrix_backward", "smil_axis_angle_to_matrix", "smil_axis_angle_to_matrix_backward",
    "smil_matrix_to_axis_angle", "smil_matrix_to_axis_angle_backward", "smil_rot6d_to_axis_angle",
    "smil_rot6d_distance", "smil_rot6d_distance_backward",
    "smil_kp_se_forward", "smil_kp_se_backward", "smil_kp_project", "smil_kp_project_backward", "smil_kp_project_loss",
    "smil_kp_project_loss_backward", "smil_kp_triangulate", "smil_kp_triangulate_backward",
    "smil_align_forward", "smil_align_backward", "smil_align_errors",
    "smil_joints_forward", "smil_joints_backward_workspace_bytes", "smil_joints_backward",
    "smil_kp3d_fit_eval_workspace_bytes", "smil_kp3d_fit_eval", "smil_adam_step_multi_bc64",
    "smil_kp2d_fit_eval_workspace_bytes", "smil_kp2d_fit_eval",
    "smil_hull_carve_workspace_bytes", "smil_hull_carve", "smil_hull_query", "smil_hull_stats", "smil_hull_surface_workspace_bytes",
    "smil_hull_surface_count", "smil_hull_surface_write",
    "smil_hull_edt_workspace_bytes", "smil_hull_edt", "smil_field_sample",
    "smil_hull_mesh_workspace_bytes", "smil_hull_mesh_count", "smil_hull_mesh_scratch_bytes", "smil_hull_mesh_write",
    "smil_point_mesh_workspace_bytes", "smil_point_face_distance", "smil_face_point_distance", "smil_point_mesh_backward",
]

N_OBJS = 10


class AdamTensor(Structure):
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("n", c_int64),
                ("lr", c_float), ("step", c_int32)]


ADAM_MAX_TENSORS = 8


class SmilError(RuntimeError):
    pass


class ModelDesc(Structure):
    _fields_ = [("V", c_int32), ("F", c_int32), ("J", c_int32), ("nB", c_int32),
                ("v_template", c_void_p), ("shapedirs", c_void_p), ("faces", c_void_p), ("parents", c_void_p),
                ("skin_idx", c_void_p), ("skin_w", c_void_p), ("jreg_rowptr", c_void_p), ("jreg_col", c_void_p),
                ("jreg_val", c_void_p), ("static_joints", c_int32), ("J_static", c_void_p), ("posedirs", c_void_p)]


class LbsInputs(Structure):
    _fields_ = [("B", c_int32), ("shared_beta", c_int32), ("nB_used", c_int32), ("beta", c_void_p),
                ("theta", c_void_p), ("Rs_in", c_void_p), ("logscale", c_void_p), ("logscale_shared", c_int32),
                ("btrans", c_void_p), ("btrans_shared", c_int32), ("trans", c_void_p), ("trans_after_joints", c_int32),
                ("del_v", c_void_p),
                ("v_template", c_void_p), ("propagate_scaling", c_int32), ("allow_limb_scaling", c_int32), ("theta_mask", c_void_p)]


class LbsOutputs(Structure):
    _fields_ = [(n, c_void_p) for n in ("v_shaped", "J_rest", "Rs", "G", "A", "new_J", "verts", "joints", "v_posed")]


class LbsGrads(Structure):
    _fields_ = [(n, c_void_p) for n in ("d_verts", "d_joints", "d_beta", "d_theta", "d_logscale", "d_btrans",
                                        "d_trans", "d_A", "d_Jrest", "d_Rs", "d_vposed", "d_posefeat", "d_del_v", "d_Rs_in")] + [
        ("accumulate_shared_beta", c_int32), ("up_Rs", c_void_p), ("up_v_shaped", c_void_p), ("clip_depth", c_void_p),
        ("beta_rows", c_void_p)]


class ClipDepth(Structure):
    _fields_ = [("vertex", c_void_p), ("dz", c_void_p), ("range", c_void_p), ("counter", c_void_p), ("capacity", c_int32)]


class Cameras(Structure):
    _fields_ = [("N", c_int32), ("views", c_int32), ("S", c_int32), ("R", c_void_p), ("nR", c_int32),
                ("T", c_void_p), ("nT", c_int32), ("fov", c_void_p), ("nFov", c_int32), ("aspect", c_void_p),
                ("nAspect", c_int32), ("principal", c_void_p), ("nPrincipal", c_int32)]


class RasterSettings(Structure):
    _fields_ = [("blur_radius", c_float), ("sigma", c_float), ("faces_per_pixel", c_int32), ("z_clip", c_float),
                ("tie_rule", c_int32), ("clip_depth", c_void_p), ("image0", c_int32)]


class FitConfig(Structure):
    _fields_ = [("N", c_int32), ("J", c_int32), ("nB", c_int32), ("window", c_int32), ("frame0", c_int32),
                ("N_total", c_int32), ("w_j2d", c_float), ("w_reproj", c_float), ("w_betas", c_float),
                ("w_pose", c_float), ("w_limit", c_float), ("w_splay", c_float), ("w_temp", c_float),
                ("limit", c_float), ("train_global", c_int32), ("train_joints", c_int32), ("train_trans", c_int32)]


class Warp(Structure):
    _fields_ = [("src", c_void_p), ("src_is_u8", c_int32), ("N_src", c_int32), ("H", c_int32), ("W", c_int32), ("C", c_int32),
                ("out", c_void_p), ("out_is_u8", c_int32), ("planar", c_int32), ("N", c_int32), ("S_h", c_int32), ("S_w", c_int32),
                ("coord_mode", c_int32), ("interp", c_int32), ("affine", c_void_p), ("n_affine", c_int32),
                ("K", c_void_p), ("K_new", c_void_p), ("dist", c_void_p), ("n_lens", c_int32), ("clamp", c_void_p), ("n_clamp", c_int32),
                ("border", c_void_p), ("n_border", c_int32), ("scale", c_float)]


class JointTables(Structure):
    _fields_ = [(n, c_int32) for n in ("J", "nB", "P", "max_depth", "static_joints")] + [
        (n, c_void_p) for n in ("parents", "depth", "child_ptr", "child", "J0", "JB", "pair_ptr", "pair_bone", "M0", "MB", "bpair_ptr",
                                "bpair_joint", "bpair_index", "rowsum")]


class JointsInputs(Structure):
    _fields_ = [("B", c_int32), ("shared_beta", c_int32), ("nB_used", c_int32), ("beta", c_void_p), ("theta", c_void_p),
                ("logscale", c_void_p), ("logscale_shared", c_int32), ("btrans", c_void_p), ("btrans_shared", c_int32),
                ("trans", c_void_p), ("trans_after_joints", c_int32), ("propagate_scaling", c_int32), ("allow_limb_scaling", c_int32),
                ("theta_mask", c_void_p)]


class JointsGrads(Structure):
    _fields_ = [(n, c_void_p) for n in ("d_joints", "d_beta", "d_theta", "d_trans", "d_logscale", "d_btrans", "workspace")]


class HullGrid(Structure):
    _fields_ = [("N", c_int32), ("Gx", c_int32), ("Gy", c_int32), ("Gz", c_int32), ("origin", c_void_p), ("n_origin", c_int32),
                ("voxel_size", c_void_p), ("n_voxel_size", c_int32)]


class MeshTopology(Structure):
    _fields_ = [("V", c_int32), ("E", c_int32), ("Q", c_int32)] + [
        (n, c_void_p) for n in ("edges", "pairs", "nbr_ptr", "nbr", "inv_deg", "vpair_ptr", "vpair")]


REG_EDGE, REG_NORMAL, REG_LAPLACIAN = 1, 2, 4
KNN_MAX_K = 64  # SMIL_KNN_MAX_K
FPS_MAX_N = 16384  # SMIL_FPS_MAX_N
BALL_MAX_RADII = 4  # SMIL_BALL_MAX_RADII
E_UNSUPPORTED = -3  # SMIL_E_UNSUPPORTED
TRI_MAX_VIEWS = 32  # SMIL_TRI_MAX_VIEWS
TRI_MAX_HYP = 50  # SMIL_TRI_MAX_HYP
TRI_RANSAC, TRI_KEEP_ALL_VIEWS = 1, 2  # SMIL_TRI_RANSAC, SMIL_TRI_KEEP_ALL_VIEWS
REFINE_MIN_POINTS = 20  # SMIL_REFINE_MIN_POINTS
REFINE_CONVERGED, REFINE_STEP_LIMIT, REFINE_SKIPPED, REFINE_NONFINITE = 0, 1, 2, 3  # SMIL_REFINE_*
REFINE_POINTS_FEW_VIEWS = 2  # SMIL_REFINE_POINTS_FEW_VIEWS
WARP_EXACT, WARP_RESIZE_LINEAR, WARP_RESIZE_NEAREST = 0, 1, 2  # SMIL_WARP_* coordinate modes
WARP_NEAREST, WARP_BILINEAR = 0, 1  # SMIL_WARP_* interpolation
ROT_F32, ROT_F64 = 0, 1  # SMIL_ROT_* dtype codes
KP_TARGET_IN_UNIT, KP_PRED_NAN_TO_ZERO, KP_FINITE_NONZERO, KP_NO_TRAILING_EPS = 1, 2, 4, 8  # SMIL_KP_* flags
KP_POOLED, KP_VALID_SAMPLES, KP_SAMPLES = 0, 1, 2  # SMIL_KP_* reductions
ALIGN_OK, ALIGN_DEGENERATE, ALIGN_EMPTY = 0, 1, 2  # SMIL_ALIGN_* status
ALIGN_NONE, ALIGN_RIGID, ALIGN_SIMILARITY = 0, 1, 2  # SMIL_ALIGN_* modes of smil_align_errors
ALIGN_SAVED = 40  # SMIL_ALIGN_SAVED
HULL_MAX_VIEWS = 64  # SMIL_HULL_MAX_VIEWS
HULL_STATS = 16  # SMIL_HULL_STATS
EDT_NONE = 2147483647  # SMIL_EDT_NONE

_lib = None


def load():
    """Load the shared library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmilError(
            f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C smilify_amd/csrc). There is no CPU fallback.")
    import torch  # noqa: F401  the library must bind to the HIP runtime torch has loaded, not bring up a second one
    lib = ctypes.CDLL(LIB_PATH)
    lib.smil_last_error.restype = c_char_p
    lib.smil_version.restype = c_char_p
    lib.smil_model_create.argtypes = [POINTER(ModelDesc), POINTER(c_void_p)]
    lib.smil_model_destroy.argtypes = [c_void_p]
    lib.smil_model_destroy.restype = None
    lib.smil_model_dims.argtypes = [c_void_p, POINTER(c_int32)]
    lib.smil_lbs_forward.argtypes = [c_void_p, POINTER(LbsInputs), POINTER(LbsOutputs), c_void_p]
    lib.smil_lbs_forward_project.argtypes = [c_void_p, POINTER(LbsInputs), POINTER(LbsOutputs), POINTER(Cameras), c_void_p, c_void_p, c_void_p]
    lib.smil_lbs_backward.argtypes = [c_void_p, POINTER(LbsInputs), POINTER(LbsOutputs), POINTER(LbsGrads), c_void_p]
    lib.smil_lbs_backward_ndc.argtypes = [c_void_p, POINTER(LbsInputs), POINTER(LbsOutputs), POINTER(LbsGrads), POINTER(Cameras),
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_lbs_backward_ndc_supported.argtypes = [c_void_p, c_int32, c_int32]
    lib.smil_clip_depth_backward.argtypes = [POINTER(Cameras), POINTER(ClipDepth), c_int32, c_int32, c_void_p, c_void_p]
    lib.smil_project.argtypes = [POINTER(Cameras), c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.smil_project_backward.argtypes = [POINTER(Cameras), c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int32, c_void_p, c_void_p]
    lib.smil_fov_reduce.argtypes = [POINTER(Cameras), c_void_p, c_void_p, c_void_p]
    lib.smil_project2.argtypes = [POINTER(Cameras), c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.smil_project_backward2.argtypes = [POINTER(Cameras), c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_fit_epilogue.argtypes = [POINTER(FitConfig)] + [c_void_p] * 12 + [c_int32, c_void_p, c_void_p, c_int32, POINTER(Cameras),
                                                                                 c_void_p, c_void_p, c_void_p]
    lib.smil_raster_workspace_bytes.argtypes = [c_void_p, c_int32, c_int32]
    lib.smil_raster_workspace_bytes.restype = c_size_t
    lib.smil_raster_stats.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_silhouette_forward.argtypes = [c_void_p, c_void_p, c_int32, c_int32, POINTER(RasterSettings), c_void_p,
                                            c_void_p, c_void_p]
    lib.smil_silhouette_backward.argtypes = [c_void_p, c_void_p, c_int32, c_int32, POINTER(RasterSettings), c_void_p,
                                             c_void_p, c_void_p, c_void_p]
    lib.smil_silhouette_l1_fused.argtypes = [c_void_p, c_void_p, c_int32, c_int32, POINTER(RasterSettings), c_void_p, c_int32,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_prior_losses.argtypes = [POINTER(FitConfig)] + [c_void_p] * 12 + [c_int32, c_void_p]
    lib.smil_mask_rows.argtypes = [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]
    lib.smil_joint_loss.argtypes = [POINTER(FitConfig), c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]
    lib.smil_pix_scale.argtypes = [POINTER(FitConfig), c_int32, c_int32, c_void_p, c_void_p]
    lib.smil_image_abs_sum.argtypes = [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.smil_sil_objective.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    lib.smil_window_terms.argtypes = [POINTER(FitConfig), c_int32, c_int32] + [c_void_p] * 10 + [c_int32, c_void_p]
    lib.smil_adam_step.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_double, c_double, c_float,
                                   c_int32, c_void_p]
    lib.smil_adam_step_multi.argtypes = [POINTER(AdamTensor), c_int32, c_double, c_double, c_float, c_void_p]
    lib.smil_adam_step_dev.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_double, c_double, c_float,
                                       c_void_p, c_int32, c_void_p]
    lib.smil_colour_workspace_bytes.argtypes = [c_void_p, c_int32, c_int32]
    lib.smil_colour_workspace_bytes.restype = c_size_t
    lib.smil_render_colour.argtypes = [c_void_p, POINTER(Cameras), c_void_p, c_void_p, POINTER(c_float), c_void_p, c_void_p, c_void_p,
                                       c_void_p]
    lib.smil_fragments_workspace_bytes.argtypes = [c_void_p, c_int32, c_int32]
    lib.smil_fragments_workspace_bytes.restype = c_size_t
    lib.smil_render_fragments.argtypes = [c_void_p, POINTER(Cameras)] + [c_void_p] * 8
    lib.smil_depth_visibility.argtypes = [c_void_p, c_int32, c_int32, c_double, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                          c_double, c_int32, c_void_p, c_void_p, c_void_p]
    lib.smil_sample_points.argtypes = [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_void_p, c_void_p,
                                       c_void_p]
    lib.smil_chamfer_workspace_bytes.argtypes = [c_int32, c_int32, c_int32]
    lib.smil_chamfer_workspace_bytes.restype = c_size_t
    lib.smil_chamfer.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 7
    lib.smil_mesh_reg_workspace_bytes.argtypes = [POINTER(MeshTopology), c_int32]
    lib.smil_mesh_reg_workspace_bytes.restype = c_size_t
    lib.smil_mesh_regularisers.argtypes = [POINTER(MeshTopology), c_void_p, c_int32, c_int32] + [c_void_p] * 6
    lib.smil_knn_workspace_bytes.argtypes = [c_int32] * 4
    lib.smil_knn_workspace_bytes.restype = c_size_t
    lib.smil_knn.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 6
    lib.smil_sdf_distance_workspace_bytes.argtypes = [c_int32] * 4
    lib.smil_sdf_distance_workspace_bytes.restype = c_size_t
    lib.smil_sdf_distance.argtypes = [c_void_p] * 4 + [c_int32] * 7 + [c_void_p] * 9
    lib.smil_sample_vertices.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_sample_vertices_backward_workspace_bytes.argtypes = [c_int32, c_int32]
    lib.smil_sample_vertices_backward_workspace_bytes.restype = c_size_t
    lib.smil_sample_vertices_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                  c_void_p]
    lib.smil_ray_diameters_workspace_bytes.argtypes = [c_int32] * 3
    lib.smil_ray_diameters_workspace_bytes.restype = c_size_t
    lib.smil_ray_diameters.argtypes = [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_float,
                                       c_float, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_fps.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.smil_ball_query.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_double), POINTER(c_int32),
                                    POINTER(c_void_p), c_void_p]
    lib.smil_group_points.argtypes = [c_void_p] * 4 + [c_int32] * 6 + [c_void_p, c_void_p]
    lib.smil_group_points_backward_workspace_bytes.argtypes = [c_int32] * 3
    lib.smil_group_points_backward_workspace_bytes.restype = c_size_t
    lib.smil_group_points_backward.argtypes = [c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p, c_void_p, c_void_p]
    lib.smil_triangulate.argtypes = [c_void_p] * 6 + [c_int64, c_int32, c_int32, c_double, c_int32, c_double, c_int32] + [c_void_p] * 8
    lib.smil_refine_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.smil_refine_workspace_bytes.restype = c_size_t
    lib.smil_refine_evaluate.argtypes = [c_void_p] * 4 + [c_int32, c_void_p, c_int32, c_double] + [c_void_p] * 5
    lib.smil_refine_cameras.argtypes = [c_void_p] * 4 + [c_int32, c_void_p, c_int32, c_double, c_int32] + [c_void_p] * 9
    lib.smil_refine_points_evaluate.argtypes = [c_void_p] * 4 + [c_int64, c_int32, c_int32, c_double] + [c_void_p] * 4
    lib.smil_refine_points.argtypes = [c_void_p] * 4 + [c_int64, c_int32, c_int32, c_double, c_int32] + [c_void_p] * 8
    lib.smil_image_bounds.argtypes = [c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p]
    lib.smil_warp_images.argtypes = [POINTER(Warp), c_void_p]
    for name in ("smil_rot6d_to_matrix", "smil_axis_angle_to_matrix", "smil_matrix_to_axis_angle", "smil_rot6d_to_axis_angle"):
        getattr(lib, name).argtypes = [c_void_p, c_void_p, c_int64, c_int32, c_void_p]
    for name in ("smil_rot6d_to_matrix_backward", "smil_axis_angle_to_matrix_backward", "smil_matrix_to_axis_angle_backward",
                 "smil_rot6d_distance"):
        getattr(lib, name).argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]
    lib.smil_rot6d_distance_backward.argtypes = [c_void_p] * 5 + [c_int64, c_int32, c_void_p]
    lib.smil_kp_se_forward.argtypes = [c_void_p] * 5 + [c_int64] + [c_int32] * 5 + [c_void_p] * 4
    lib.smil_kp_se_backward.argtypes = [c_void_p] * 8 + [c_int64] + [c_int32] * 4 + [c_void_p]
    lib.smil_kp_project.argtypes = [c_void_p] * 5 + [c_int64, c_int32, c_int32, c_double, c_int32, c_void_p, c_void_p]
    lib.smil_kp_project_backward.argtypes = [c_void_p] * 6 + [c_int64, c_int32, c_int32, c_double, c_int32] + [c_void_p] * 5
    lib.smil_kp_project_loss.argtypes = [c_void_p] * 9 + [c_int64, c_int32, c_int32, c_double, c_int32] + [c_void_p] * 4
    lib.smil_kp_project_loss_backward.argtypes = [c_void_p] * 11 + [c_int64, c_int32, c_int32, c_double, c_int32] + [c_void_p] * 5
    lib.smil_kp_triangulate.argtypes = [c_void_p] * 7 + [c_int64, c_int32, c_int32, c_double, c_double, c_double, c_int32] + [c_void_p] * 4
    lib.smil_kp_triangulate_backward.argtypes = [c_void_p] * 8 + [c_int64, c_int32, c_int32, c_double, c_double, c_int32] + [c_void_p] * 5
    lib.smil_align_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_int32, c_double, c_int32, c_double,
                                       c_int32] + [c_void_p] * 9
    lib.smil_align_backward.argtypes = [c_void_p] * 8 + [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.smil_align_errors.argtypes = [c_void_p] * 3 + [c_int64, c_int32, c_int32, c_int32, c_double, c_double, c_int32] + [c_void_p] * 4
    lib.smil_joints_forward.argtypes = [POINTER(JointTables), POINTER(JointsInputs), c_void_p, c_void_p, c_void_p]
    lib.smil_joints_backward_workspace_bytes.argtypes = [POINTER(JointTables), POINTER(JointsInputs), POINTER(JointsGrads)]
    lib.smil_joints_backward_workspace_bytes.restype = c_size_t
    lib.smil_joints_backward.argtypes = [POINTER(JointTables), POINTER(JointsInputs), POINTER(JointsGrads), c_void_p]
    lib.smil_kp3d_fit_eval_workspace_bytes.argtypes = [POINTER(JointTables), POINTER(JointsInputs), c_int32, c_int32, c_int32]
    lib.smil_kp3d_fit_eval_workspace_bytes.restype = c_size_t
    lib.smil_kp3d_fit_eval.argtypes = [POINTER(FitConfig), c_double, c_double, POINTER(JointTables), POINTER(JointsInputs), c_int32] + \
        [c_void_p] * 13
    lib.smil_kp2d_fit_eval_workspace_bytes.argtypes = [POINTER(JointTables), POINTER(JointsInputs), POINTER(Cameras), c_int32, c_int32, c_int32]
    lib.smil_kp2d_fit_eval_workspace_bytes.restype = c_size_t
    lib.smil_kp2d_fit_eval.argtypes = [POINTER(FitConfig), c_double, c_double, POINTER(JointTables), POINTER(JointsInputs), POINTER(Cameras),
                                       c_int32] + [c_void_p] * 5 + [c_double, c_double] + [c_void_p] * 12
    lib.smil_adam_step_multi_bc64.argtypes = [POINTER(AdamTensor), c_int32, c_double, c_double, c_float, c_void_p]
    lib.smil_hull_carve_workspace_bytes.argtypes = [POINTER(HullGrid)]
    lib.smil_hull_carve_workspace_bytes.restype = c_size_t
    lib.smil_hull_carve.argtypes = [POINTER(HullGrid), c_void_p, c_int32, c_int32, c_int32, c_float, POINTER(Cameras), c_int32, c_int32, c_int32] + \
        [c_void_p] * 5
    lib.smil_hull_query.argtypes = [c_void_p, c_int32, c_int64, c_void_p, c_int32, c_int32, c_int32, c_float, POINTER(Cameras), c_int32] + \
        [c_void_p] * 3
    lib.smil_hull_stats.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p]
    lib.smil_hull_surface_workspace_bytes.argtypes = [POINTER(HullGrid)]
    lib.smil_hull_surface_workspace_bytes.restype = c_size_t
    lib.smil_hull_surface_count.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_hull_surface_write.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_hull_edt_workspace_bytes.argtypes = [POINTER(HullGrid)]
    lib.smil_hull_edt_workspace_bytes.restype = c_size_t
    lib.smil_hull_edt.argtypes = [POINTER(HullGrid), c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.smil_field_sample.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_hull_mesh_workspace_bytes.argtypes = [POINTER(HullGrid)]
    lib.smil_hull_mesh_workspace_bytes.restype = c_size_t
    lib.smil_hull_mesh_count.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.smil_hull_mesh_scratch_bytes.argtypes = [c_int64, c_int32]
    lib.smil_hull_mesh_scratch_bytes.restype = c_size_t
    lib.smil_hull_mesh_write.argtypes = [POINTER(HullGrid), c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p]
    lib.smil_point_mesh_workspace_bytes.argtypes = [c_int32] * 4
    lib.smil_point_mesh_workspace_bytes.restype = c_size_t
    _pm = [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32] + [c_void_p] * 5
    lib.smil_point_face_distance.argtypes = _pm
    lib.smil_face_point_distance.argtypes = _pm
    lib.smil_point_mesh_backward.argtypes = [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                             c_void_p, c_int32] + [c_void_p] * 6
    lib.smil_profile_enable.argtypes = [c_int32]
    lib.smil_profile_read.argtypes = [POINTER(c_float), POINTER(c_int32)]
    for name in EXPORTS:
        fn = getattr(lib, name)  # raises AttributeError if the symbol is missing
        if fn.restype is ctypes.c_int:
            fn.restype = c_int32
    _lib = lib
    return lib


def check(rc: int, what: str = "libsmilfit call") -> None:
    if rc != 0:
        msg = load().smil_last_error()
        raise SmilError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
