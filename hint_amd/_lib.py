"""ctypes binding of libhint_amd.so (the C ABI declared in include/hint_amd.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, the
caller gets an exception.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C hint_amd/csrc`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HINT_AMD_LIB") or os.path.join(_HERE, "lib", "libhint_amd.so")
ABI_VERSION = 8


class HintAmdError(RuntimeError):
    pass


class AdamSeg(C.Structure):
    """mirror of `hint_adam_seg` (include/hint_amd.h)"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class NodeDesc(C.Structure):
    """mirror of `hint_node_desc` (include/hint_amd.h)"""
    _fields_ = [("off", C.c_int32), ("D", C.c_int32), ("k", C.c_int32), ("r", C.c_int32),
                ("h", C.c_int32), ("depth", C.c_int32), ("p_off", C.c_int64 * 12)]


class MmdDesc(C.Structure):
    """mirror of `hint_mmd_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("n_x", C.c_int32), ("n_y", C.c_int32), ("d", C.c_int32),
                ("n_kernels", C.c_int32), ("width", C.c_float * 8), ("exponent", C.c_float * 8), ("yy", C.c_void_p),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class AbcDesc(C.Structure):
    """mirror of `hint_abc_desc` (include/hint_amd.h)"""
    _fields_ = [("y", C.c_void_p), ("target", C.c_void_p), ("n_rows", C.c_int64), ("ny", C.c_int32), ("k", C.c_int32),
                ("idx", C.c_void_p), ("dist", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class CurveDesc(C.Structure):
    """mirror of `hint_curve_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32), ("n_points", C.c_int32),
                ("eps", C.c_void_p), ("noise", C.c_float), ("target", C.c_void_p), ("y", C.c_void_p), ("dist", C.c_void_p),
                ("mean", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("max_groups", C.c_int32)]


class HausdorffDesc(C.Structure):
    """mirror of `hint_hausdorff_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("b_points", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32),
                ("n_points", C.c_int32), ("a_points", C.c_void_p), ("a_offsets", C.c_void_p), ("a_params", C.c_void_p),
                ("n_template", C.c_int64), ("max_h", C.c_void_p), ("avg_h", C.c_void_p), ("chamfer", C.c_void_p),
                ("points", C.c_void_p), ("max_groups", C.c_int32)]


class PlusDesc(C.Structure):
    """mirror of `hint_plus_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("b_points", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32),
                ("n_points", C.c_int32), ("params", C.c_void_p), ("max_dist", C.c_float), ("max_groups", C.c_int32),
                ("segments", C.c_void_p), ("keep", C.c_void_p), ("counts", C.c_void_p), ("loss", C.c_void_p),
                ("max_h", C.c_void_p), ("avg_h", C.c_void_p)]


class LensFitDesc(C.Structure):
    """mirror of `hint_lensfit_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("b_points", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32),
                ("n_points", C.c_int32), ("a_points", C.c_void_p), ("n_template", C.c_int64), ("starts", C.c_void_p),
                ("n_starts", C.c_int32), ("n_steps", C.c_int32), ("lr", C.c_double), ("angle_lr", C.c_double),
                ("gamma", C.c_double), ("momentum", C.c_double), ("weight", C.c_double), ("params", C.c_void_p),
                ("loss", C.c_void_p), ("best", C.c_void_p), ("all_params", C.c_void_p), ("all_loss", C.c_void_p),
                ("grad", C.c_void_p), ("trace", C.c_void_p), ("max_groups", C.c_int32)]


class PlusFitDesc(C.Structure):
    """mirror of `hint_plusfit_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("b_points", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32),
                ("n_points", C.c_int32), ("starts", C.c_void_p), ("n_starts", C.c_int32), ("n_steps", C.c_int32),
                ("lr", C.c_double), ("angle_lr", C.c_double), ("gamma", C.c_double), ("momentum", C.c_double),
                ("corner_weight", C.c_double), ("stop_loss", C.c_double), ("corner_decay", C.c_int32),
                ("max_groups", C.c_int32), ("params", C.c_void_p), ("loss", C.c_void_p), ("best", C.c_void_p),
                ("n_run", C.c_void_p), ("all_params", C.c_void_p), ("all_loss", C.c_void_p), ("grad", C.c_void_p),
                ("trace", C.c_void_p)]


class OverlapDesc(C.Structure):
    """mirror of `hint_overlap_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("b_points", C.c_void_p), ("n_rows", C.c_int64), ("n_coeffs", C.c_int32),
                ("n_points", C.c_int32), ("a_points", C.c_void_p), ("a_offsets", C.c_void_p), ("a_params", C.c_void_p),
                ("n_template", C.c_int64), ("plus_params", C.c_void_p), ("areas", C.c_void_p), ("iou", C.c_void_p),
                ("dice", C.c_void_p), ("crossings", C.c_void_p), ("max_groups", C.c_int32)]


class CorrDesc(C.Structure):
    """mirror of `hint_corr_desc` (include/hint_amd.h)"""
    _fields_ = [("x", C.c_void_p), ("n", C.c_int32), ("d", C.c_int32), ("target", C.c_void_p), ("corr", C.c_void_p),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class LensGenDesc(C.Structure):
    """mirror of `hint_lensgen_desc` (include/hint_amd.h)"""
    _fields_ = [("n_rows", C.c_int64), ("seed", C.c_uint64), ("offset", C.c_uint64), ("draws", C.c_void_p), ("x", C.c_void_p),
                ("ring", C.c_void_p), ("counts", C.c_void_p), ("eps", C.c_void_p), ("draws_out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("max_groups", C.c_int32)]


class FcoefDesc(C.Structure):
    """mirror of `hint_fcoef_desc` (include/hint_amd.h)"""
    _fields_ = [("points", C.c_void_p), ("counts", C.c_void_p), ("n_rows", C.c_int64), ("p_max", C.c_int32),
                ("n_coeffs", C.c_int32), ("x", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("max_groups", C.c_int32)]


class PlusGenDesc(C.Structure):
    """mirror of `hint_plusgen_desc` (include/hint_amd.h); the stream is a field, not a parameter of the run"""
    _fields_ = [("n_rows", C.c_int64), ("seed", C.c_uint64), ("offset", C.c_uint64), ("rows", C.c_void_p), ("draws", C.c_void_p),
                ("target", C.POINTER(C.c_float)), ("x", C.c_void_p), ("y", C.c_void_p), ("outline", C.c_void_p),
                ("counts", C.c_void_p), ("corners", C.c_void_p), ("draws_out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("max_groups", C.c_int32), ("stream", C.c_void_p)]


class HouseholderDesc(C.Structure):
    """mirror of `hint_householder_desc` (include/hint_amd.h); the stream is a field, not a parameter of the run"""
    _fields_ = [("op", C.c_int32), ("transpose", C.c_int32), ("B", C.c_int32), ("d", C.c_int32), ("n", C.c_int32),
                ("Vs", C.c_void_p), ("W", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("g_y", C.c_void_p),
                ("g_x", C.c_void_p), ("g_W", C.c_void_p), ("g_V", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


HOUSEHOLDER_BUILD, HOUSEHOLDER_APPLY, HOUSEHOLDER_GRAD = 0, 1, 2


class HouseholderMany(C.Structure):
    """mirror of `hint_householder_many` (include/hint_amd.h); the stream is a field, not a parameter of the run"""
    _fields_ = [("op", C.c_int32), ("m", C.c_int32), ("j", C.c_int32), ("B", C.c_int32), ("d", C.c_int32), ("n", C.c_int32),
                ("Vs", C.c_void_p), ("vs_stride", C.c_int64), ("W", C.c_void_p), ("w_stride", C.c_int64), ("x", C.c_void_p),
                ("g_y", C.c_void_p), ("g_x", C.c_void_p), ("g_W", C.c_void_p), ("gw_stride", C.c_int64), ("g_V", C.c_void_p),
                ("gv_stride", C.c_int64), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("ws_stride", C.c_int64),
                ("stream", C.c_void_p)]


HOUSEHOLDER_MANY_BUILD, HOUSEHOLDER_MANY_ROWS, HOUSEHOLDER_MANY_FINISH = 0, 1, 2


class EpochDesc(C.Structure):
    """mirror of `hint_epoch_desc` (include/hint_amd.h); the stream is a field, not a parameter of the run"""
    _fields_ = [("op", C.c_int32), ("shuffle", C.c_int32), ("d", C.c_int32), ("dy", C.c_int32), ("epoch", C.c_uint32),
                ("max_groups", C.c_int32), ("n_rows", C.c_int64), ("seed", C.c_uint64), ("first", C.c_int64), ("count", C.c_int64),
                ("block", C.c_int64), ("block_stride", C.c_int64), ("x", C.c_void_p), ("x_stride", C.c_int64), ("y", C.c_void_p),
                ("y_stride", C.c_int64), ("cursor", C.c_void_p), ("out_x", C.c_void_p), ("out_stride", C.c_int64),
                ("out_y", C.c_void_p), ("indices_out", C.c_void_p), ("mean", C.c_void_p), ("std", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


EPOCH_GATHER, EPOCH_MOMENTS, EPOCH_STANDARDIZE = 0, 1, 2

_lib = None

_PROTOS = {
    "hint_abi_version": (C.c_int, []),
    "hint_last_error": (C.c_char_p, []),
    "hint_build_info": (C.c_char_p, []),
    "hint_debug_set_prefetch": (C.c_int, [C.c_int]),
    "hint_debug_reload_knobs": (C.c_int, []),
    "hint_debug_last_lds_bytes": (C.c_int32, [C.c_int32]),
    "hint_debug_last_wl_shape": (C.c_int32, [C.c_int32]),
    "hint_plan_create": (C.c_int, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                   C.POINTER(C.c_void_p)]),
    "hint_plan_check": (C.c_int, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                  C.POINTER(C.c_int64)]),
    "hint_plan_destroy": (None, [C.c_void_p]),
    "hint_plan_param_floats": (C.c_int64, [C.c_void_p]),
    "hint_plan_packed_floats": (C.c_int64, [C.c_void_p]),
    "hint_plan_tape_floats": (C.c_int64, [C.c_void_p, C.c_int32]),
    "hint_plan_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "hint_plan_lds_bytes": (C.c_int32, [C.c_void_p, C.c_int32]),
    "hint_plan_describe": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "hint_plan_dispatch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "hint_plan_check_dispatch": (C.c_int, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                           C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "hint_plan_paths": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "hint_plan_check_paths": (C.c_int, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                        C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "hint_plan_check_wl_shape": (C.c_int64, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "hint_plan_check_digest": (C.c_int, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                         C.POINTER(C.c_uint64), C.c_int32]),
    "hint_plan_check_wjob": (C.c_int64, [C.POINTER(NodeDesc), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int64,
                                         C.c_int32]),
    "hint_block_pack": (C.c_int, [C.c_void_p] * 4),
    "hint_pack_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.c_int32, C.POINTER(C.c_void_p)]),
    "hint_pack_group_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hint_pack_group_run_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hint_pack_group_destroy": (None, [C.c_void_p]),
    "hint_block_forward": (C.c_int, [C.c_void_p] * 8 + [C.c_int32, C.c_void_p]),
    "hint_block_inverse": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]),
    "hint_block_backward": (C.c_int, [C.c_void_p] * 11 + [C.c_int32, C.c_void_p, C.c_size_t, C.c_int32,
                                                          C.c_void_p]),
    "hint_block_forward_ex": (C.c_int, [C.c_void_p] * 11 + [C.c_int32, C.c_void_p]),
    "hint_block_inverse_ex": (C.c_int, [C.c_void_p] * 9 + [C.c_int32, C.c_void_p]),
    "hint_block_backward_ex": (C.c_int, [C.c_void_p] * 11 + [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                             C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "hint_plan_inverse_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "hint_block_inverse_backward": (C.c_int, [C.c_void_p] * 9 + [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32,
                                                                 C.c_void_p]),
    "hint_chain_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "hint_chain_set_block": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "hint_chain_commit": (C.c_int, [C.c_void_p]),
    "hint_chain_forward": (C.c_int, [C.c_void_p] * 8),
    "hint_chain_forward_noisy": (C.c_int, [C.c_void_p] * 7 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hint_chain_backward": (C.c_int, [C.c_void_p] * 7 + [C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "hint_chain_destroy": (None, [C.c_void_p]),
    "hint_chain_backward_adam": (C.c_int, [C.c_void_p] * 7 + [C.c_float, C.c_float] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]
                                 + [C.c_float] * 6 + [C.c_void_p]),
    "hint_chain_backward_parts": (C.c_int, [C.c_void_p] * 7 + [C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "hint_chain_wgrad_range": (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hint_chain_inverse": (C.c_int, [C.c_void_p] * 7),
    "hint_chain_set_block_io": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hint_chain_wgrad_adam": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p] + [C.c_float] * 6 + [C.c_void_p]),
    "hint_block_forward_noisy": (C.c_int, [C.c_void_p] * 11 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "hint_block_backward_rows": (C.c_int, [C.c_void_p] * 11 + [C.c_size_t, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "hint_block_ext_coeffs": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p]),
    "hint_chain_set_block_affine": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "hint_adam_step_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_void_p] + [C.c_float] * 6 + [C.c_int32, C.c_void_p]),
    "hint_adam_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int32] + [C.c_float] * 7 + [C.c_int32,
                                                                                                 C.c_void_p]),
    "hint_adam_multi_create": (C.c_int, [C.POINTER(AdamSeg), C.c_int32, C.POINTER(C.c_void_p)]),
    "hint_adam_multi_step": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_float] * 7 + [C.c_int32, C.c_void_p]),
    "hint_adam_multi_destroy": (None, [C.c_void_p]),
    "hint_adam_multi_chunk": (C.c_int64, [C.POINTER(AdamSeg), C.c_int32, C.c_int64, C.c_int32]),
    "hint_mmd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "hint_mmd_run": (C.c_int, [C.POINTER(MmdDesc), C.c_void_p]),
    "hint_mmd_job": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "hint_abc_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_abc_run": (C.c_int, [C.POINTER(AbcDesc), C.c_void_p]),
    "hint_abc_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_curve_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_curve_run": (C.c_int, [C.POINTER(CurveDesc), C.c_void_p]),
    "hint_curve_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "hint_hausdorff_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "hint_hausdorff_run": (C.c_int, [C.POINTER(HausdorffDesc), C.c_void_p]),
    "hint_hausdorff_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "hint_plus_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_plus_run": (C.c_int, [C.POINTER(PlusDesc), C.c_void_p]),
    "hint_plus_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_lensfit_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "hint_lensfit_run": (C.c_int, [C.POINTER(LensFitDesc), C.c_void_p]),
    "hint_lensfit_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_plusfit_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "hint_plusfit_run": (C.c_int, [C.POINTER(PlusFitDesc), C.c_void_p]),
    "hint_plusfit_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_overlap_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "hint_overlap_run": (C.c_int, [C.POINTER(OverlapDesc), C.c_void_p]),
    "hint_overlap_geometry": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "hint_corr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "hint_corr_run": (C.c_int, [C.POINTER(CorrDesc), C.c_void_p]),
    "hint_corr_job": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "hint_lensgen_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "hint_lensgen_run": (C.c_int, [C.POINTER(LensGenDesc), C.c_void_p]),
    "hint_fcoef_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "hint_fcoef_run": (C.c_int, [C.POINTER(FcoefDesc), C.c_void_p]),
    "hint_plusgen_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "hint_plusgen_run": (C.c_int, [C.POINTER(PlusGenDesc)]),
    "hint_householder_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "hint_householder_run": (C.c_int, [C.POINTER(HouseholderDesc)]),
    "hint_householder_geometry": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "hint_householder_many_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "hint_householder_many_run": (C.c_int, [C.POINTER(HouseholderMany)]),
    "hint_epoch_index": (C.c_int64, [C.c_int64, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64]),
    "hint_epoch_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "hint_epoch_run": (C.c_int, [C.POINTER(EpochDesc)]),
}


def exported_symbols():
    """names every entry point include/hint_amd.h declares (used by the symbol test)"""
    return sorted(_PROTOS)


def load():
    """Load the library once; raise HintAmdError loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HintAmdError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build() or `make -C hint_amd/csrc`). There is no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. ROCm runtime missing
        raise HintAmdError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)      # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    if lib.hint_abi_version() != ABI_VERSION:
        raise HintAmdError(f"ABI version mismatch: library {lib.hint_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int, what: str):
    if status != 0:
        msg = load().hint_last_error()
        raise HintAmdError(f"{what} failed: {msg.decode() if msg else 'unknown error'}")
