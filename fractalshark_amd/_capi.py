"""ctypes declarations for the two native libraries.  No torch types cross these boundaries."""
import ctypes as C
import os

from . import _build

vp = C.c_void_p
u32 = C.c_uint32
u64 = C.c_uint64
i32 = C.c_int32


class RealHdr32(C.Structure):
    _fields_ = [("m", C.c_float), ("e", C.c_int32)]


class CplxHdr32(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float), ("e", C.c_int32)]


class AtHdr32(C.Structure):
    _fields_ = [("StepLength", u32), ("ThresholdC", RealHdr32), ("SqrEscapeRadius", RealHdr32),
                ("RefC", CplxHdr32), ("ZCoeff", CplxHdr32), ("CCoeff", CplxHdr32), ("InvZCoeff", CplxHdr32),
                ("CCoeffSqrInvZCoeff", CplxHdr32), ("CCoeffInvZCoeff", CplxHdr32),
                ("CCoeffNormSqr", RealHdr32), ("RefCNormSqr", RealHdr32), ("factor", RealHdr32)]


class Reduction(C.Structure):
    _fields_ = [("Min", u64), ("Max", u64), ("Sum", u64)]


class RealHdr64(C.Structure):
    _fields_ = [("m", C.c_double), ("e", C.c_int32), ("pad_", C.c_int32)]


class CplxHdr64(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double), ("e", C.c_int32), ("pad_", C.c_int32)]


class AtHdr64(C.Structure):
    _fields_ = [("StepLength", u32), ("pad_", u32), ("ThresholdC", RealHdr64), ("SqrEscapeRadius", RealHdr64),
                ("RefC", CplxHdr64), ("ZCoeff", CplxHdr64), ("CCoeff", CplxHdr64), ("InvZCoeff", CplxHdr64),
                ("CCoeffSqrInvZCoeff", CplxHdr64), ("CCoeffInvZCoeff", CplxHdr64),
                ("CCoeffNormSqr", RealHdr64), ("RefCNormSqr", RealHdr64), ("factor", RealHdr64)]


class Real2x32(C.Structure):
    _fields_ = [("head", C.c_float), ("tail", C.c_float), ("e", C.c_int32)]


class Cplx2x32(C.Structure):
    _fields_ = [("re_head", C.c_float), ("re_tail", C.c_float), ("im_head", C.c_float), ("im_tail", C.c_float),
                ("e", C.c_int32)]


class At2x32(C.Structure):
    _fields_ = [("StepLength", u32), ("ThresholdC", Real2x32), ("SqrEscapeRadius", Real2x32),
                ("RefC", Cplx2x32), ("ZCoeff", Cplx2x32), ("CCoeff", Cplx2x32), ("InvZCoeff", Cplx2x32),
                ("CCoeffSqrInvZCoeff", Cplx2x32), ("CCoeffInvZCoeff", Cplx2x32),
                ("CCoeffNormSqr", Real2x32), ("RefCNormSqr", Real2x32), ("factor", Real2x32)]


class AutozoomResult(C.Structure):
    """fs_autozoom_result (include/fs_layout.h)."""
    _fields_ = [("status", u32), ("heuristic", u32), ("target_x", C.c_double), ("target_y", C.c_double),
                ("max_iter", u64), ("num_at_limit", u64), ("num_at_max", u64), ("sum_iters", u64), ("avg", C.c_double),
                ("candidates", u64), ("accepted", u64), ("high_hist", u64 * 9), ("run_reject", u64), ("rescored", u64),
                ("score", C.c_double), ("sum_sq", C.c_double), ("sum_sq_x", C.c_double), ("sum_sq_y", C.c_double)]


class AuditOffender(C.Structure):
    """fs_audit_offender (include/fs_layout.h)."""
    _fields_ = [("sample", u32), ("stable_bits", u32), ("frame_value", u64), ("exact_value", u64)]


AUDIT_MAX_LEVELS, AUDIT_MAX_OFFENDERS = 8, 16


class AuditResult(C.Structure):
    """fs_audit_result (include/fs_layout.h)."""
    _fields_ = [("n_samples", u32), ("n_levels", u32), ("n_equal", u32), ("n_differ", u32), ("n_capped", u32), ("n_offenders", u32),
                ("stable", u32 * AUDIT_MAX_LEVELS), ("stable_differ", u32 * AUDIT_MAX_LEVELS),
                ("stable_capped", u32 * AUDIT_MAX_LEVELS), ("max_abs_diff", u64 * AUDIT_MAX_LEVELS),
                ("offenders", AuditOffender * AUDIT_MAX_OFFENDERS)]


class ExactKept(C.Structure):
    """fs_exact_kept (include/fs_layout.h)."""
    _fields_ = [("samples", u64), ("proved", u64), ("cap", u64), ("device_bytes", u64), ("frac_bits", u32), ("limbs", u32),
                ("bailout", u32), ("inclusive", u32), ("wide", u32), ("cycle_check", u32), ("valid", u32), ("reserved", u32)]


class FeatureInF32(C.Structure):
    """fs_feature_in_f32 (include/fs_layout.h)."""
    _fields_ = [("dc", C.c_float * 2), ("c", C.c_float * 2), ("period", u64)]


class FeatureInF64(C.Structure):
    """fs_feature_in_f64 (include/fs_layout.h)."""
    _fields_ = [("dc", C.c_double * 2), ("c", C.c_double * 2), ("period", u64)]


class FeatureOutF32(C.Structure):
    """fs_feature_out_f32 (include/fs_layout.h)."""
    _fields_ = [("status", u32), ("pad0_", u32), ("period", u64), ("diff", C.c_float * 2), ("dzdc", C.c_float * 2),
                ("zcoeff", C.c_float * 2), ("residual2", C.c_float), ("pad1_", u32)]


class FeatureOutF64(C.Structure):
    """fs_feature_out_f64 (include/fs_layout.h)."""
    _fields_ = [("status", u32), ("pad0_", u32), ("period", u64), ("diff", C.c_double * 2), ("dzdc", C.c_double * 2),
                ("zcoeff", C.c_double * 2), ("residual2", C.c_double)]


assert C.sizeof(FeatureInF32) == 24 and C.sizeof(FeatureInF64) == 40
assert C.sizeof(FeatureOutF32) == 48 and C.sizeof(FeatureOutF64) == 72
assert C.sizeof(ExactKept) == 64
assert C.sizeof(AutozoomResult) == 200
assert C.sizeof(AuditOffender) == 24 and C.sizeof(AuditResult) == 568
assert C.sizeof(AtHdr32) == 116 and C.sizeof(AtHdr64) == 232 and C.sizeof(At2x32) == 184

DONE_CB = C.CFUNCTYPE(None, vp)

_render = None
_inputs = None


def _decl(lib, name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


def render_lib():
    """libfsmi355.so.  Raises if the HIP library has not been built: there is no fallback."""
    global _render
    if _render is not None:
        return _render
    # FSMI355_LIB: another build of the same library (A/B measurements against other build flags; tools/c2_ab.py)
    path = os.environ.get("FSMI355_LIB") or _build.LIB_RENDER
    if os.environ.get("FSMI355_LIB"):
        # (advisor, round 5: an override has no stamp check -- at least say which build is being measured)
        import sys
        print("fractalshark_amd: FSMI355_LIB overrides the in-tree library: %s" % path, file=sys.stderr)
    if not os.path.exists(path):
        raise RuntimeError("libfsmi355.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % path)
    lib = C.CDLL(path)
    _decl(lib, "fs_create", vp, [C.c_int])
    _decl(lib, "fs_destroy", None, [vp])
    _decl(lib, "fs_test_device_is_working", u32, [])
    _decl(lib, "fs_device_count", C.c_int, [])
    _decl(lib, "fs_host_fallback_bytes", u64, [vp])
    _decl(lib, "fs_idle_device_bytes", u64, [vp])
    _decl(lib, "fs_release_idle_device_memory", u64, [C.c_int])
    _decl(lib, "fs_set_compressed_orbit_mode", u32, [vp, C.c_int])
    _decl(lib, "fs_orbit_device_bytes", u64, [vp])
    _decl(lib, "fs_error_string", C.c_char_p, [u32])
    _decl(lib, "fs_init_memory", u32, [vp, u32, u32, u32, u32, vp, u32, u32, u64, C.c_int])
    _decl(lib, "fs_set_row_bands", u32, [vp, u32, u32, u32])
    _decl(lib, "fs_local_rows", u32, [vp])
    _decl(lib, "fs_set_external_iter_buffer", u32, [vp, vp, u64])
    _decl(lib, "fs_device_iter_buffer", vp, [vp])
    _decl(lib, "fs_rounded_width", u32, [vp])
    _decl(lib, "fs_upload_orbit", u32, [vp, u64, C.c_int, u32, vp, u64, u64, u64])
    _decl(lib, "fs_upload_orbit_compressed", u32, [vp, u64, C.c_int, u32, vp, u64, u64, u64, vp, vp])
    _decl(lib, "fs_upload_la", u32, [vp, u64, C.c_int, u32, vp, u32, vp, u32, C.c_int, C.c_int, vp])
    _decl(lib, "fs_upload_bla", u32, [vp, C.c_int, vp, vp, i32, i32])
    _decl(lib, "fs_render_lav2", u32, [vp, C.c_int, C.c_int, C.c_int, vp, u64])
    _decl(lib, "fs_feature_eval", u32, [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64])
    _decl(lib, "fs_feature_eval_direct", u32, [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64])
    _decl(lib, "fs_feature_eval_resident", u32, [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64])
    _decl(lib, "fs_feature_eval_plain", u32, [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64])
    _decl(lib, "fs_feature_eval_plain_direct", u32, [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64])
    _decl(lib, "fs_orbit_form", C.c_int, [vp])
    _decl(lib, "fs_set_feature_slice", u32, [vp, u32])
    _decl(lib, "fs_autozoom_pick", u32, [vp, C.c_int, u64, vp, C.POINTER(AutozoomResult)])
    _decl(lib, "fs_set_autozoom_gather_cap", u32, [vp, u32])
    _decl(lib, "fs_render_exact", u32, [vp, u32, u32, u32, vp, vp, u32, C.c_int, u64])
    _decl(lib, "fs_exact_stable_mask", u32, [vp, u32, u32, vp, vp, u32, u64, vp])
    _decl(lib, "fs_set_exact_slice", u32, [vp, u32, C.c_int])
    _decl(lib, "fs_read_exact_stats", u32, [vp, vp])
    _decl(lib, "fs_exact_sample_counts", u32, [vp, u32, u32, vp, vp, u32, u32, C.c_int, u64, vp])
    _decl(lib, "fs_exact_eval_points", u32, [vp, u32, u32, vp, vp, vp, u32, u32, C.c_int, vp, vp, vp, vp])
    _decl(lib, "fs_exact_eval_points_wide", u32, [vp, u32, u32, vp, vp, vp, u32, u32, C.c_int, vp, vp, vp, vp])
    _decl(lib, "fs_render_exact_wide", u32, [vp, u32, u32, u32, vp, vp, u32, C.c_int, u64])
    _decl(lib, "fs_exact_wide_state", u32, [vp, u32, u32, vp, vp, u32, u32, vp, vp])
    _decl(lib, "fs_exact_audit", u32, [vp, vp, u32, u32, vp, vp, u32, u32, vp, vp, u32, C.c_int, u64, C.POINTER(AuditResult), vp, vp, vp])
    _decl(lib, "fs_set_exact_cycle_check", u32, [vp, C.c_int])
    _decl(lib, "fs_read_exact_proved", u32, [vp, vp, u64])
    _decl(lib, "fs_read_exact_cycle_stats", u32, [vp, vp])
    _decl(lib, "fs_set_exact_cycle_fingerprint_bits", u32, [vp, u32])
    _decl(lib, "fs_set_exact_keep", u32, [vp, C.c_int])
    _decl(lib, "fs_render_exact_continue", u32, [vp, u64])
    _decl(lib, "fs_exact_kept_info", u32, [vp, C.POINTER(ExactKept)])
    _decl(lib, "fs_exact_drop_kept", u32, [vp])
    _decl(lib, "fs_set_exact_periods", u32, [vp, C.c_int])
    _decl(lib, "fs_read_exact_atom_periods", u32, [vp, vp, u64])
    _decl(lib, "fs_read_exact_cycle_lengths", u32, [vp, vp, u64])
    _decl(lib, "fs_set_exact_atom_key_bits", u32, [vp, u32])
    _decl(lib, "fs_render_bla", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_render_direct", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_upload_orbit_scaled", u32, [vp, C.c_int, u32, vp, vp, u64, u64])
    _decl(lib, "fs_render_scaled", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_build_bla", u32, [vp, C.c_int, vp])
    _decl(lib, "fs_bla_num_levels", i32, [vp])
    _decl(lib, "fs_bla_lm2", i32, [vp])
    _decl(lib, "fs_bla_level_size", u64, [vp, i32])
    _decl(lib, "fs_read_bla_level", u32, [vp, i32, vp, u64])
    _decl(lib, "fs_bla_lookup_probe", u32, [vp, C.c_int, vp, vp, u32, vp])
    _decl(lib, "fs_read_bla_native", u32, [vp, C.c_int, vp, u64, vp])
    _decl(lib, "fs_render_direct_lp", u32, [vp, C.c_int, vp, u64, C.c_int])
    _decl(lib, "fs_clear", u32, [vp])
    _decl(lib, "fs_render_current", u32, [vp, u64, vp, vp, vp, C.c_int])
    _decl(lib, "fs_sync_compute", u32, [vp])
    _decl(lib, "fs_compute_stream", vp, [vp])
    _decl(lib, "fs_sync_display", u32, [vp])
    _decl(lib, "fs_query_compute", u32, [vp])
    _decl(lib, "fs_enqueue_done_callback", u32, [vp, DONE_CB, vp])
    _decl(lib, "fs_get_width", u32, [vp])
    _decl(lib, "fs_get_height", u32, [vp])
    _decl(lib, "fs_last_kernel_ms", C.c_float, [vp])
    _decl(lib, "fs_set_kernel_variant", u32, [vp, C.c_int])
    _decl(lib, "fs_kernel_ms_history", u32, [vp, vp, u32])
    _decl(lib, "fs_kernel_ms_split_history", u32, [vp, vp, vp, u32])
    _decl(lib, "fs_forget_tile_costs", u32, [vp])
    _decl(lib, "fs_last_frame_tile_ordered", C.c_int, [vp])
    _decl(lib, "fs_last_frame_sampled_tile_order", C.c_int, [vp])
    _decl(lib, "fs_read_tile_costs", u32, [vp, vp, u64, vp])
    _decl(lib, "fs_read_tile_order", u32, [vp, vp, u64])
    _decl(lib, "fs_seq_cursor_probe", u32, [vp, C.c_int, u64, u32, vp])
    _decl(lib, "fs_enable_step_count", u32, [vp, C.c_int])
    _decl(lib, "fs_read_step_count", u32, [vp, vp])
    _decl(lib, "fs_time_render_current", u32, [vp, u64, u32, vp])
    _decl(lib, "fs_read_stats_raw", u32, [vp, vp, u64])
    _decl(lib, "fs_test_block_threshold", u32, [vp, vp, vp, vp, vp, u32])
    _decl(lib, "fs_test_ndz_threshold", u32, [vp, vp, vp, vp, vp, u32])
    _decl(lib, "fs_read_ndz_bounds", u32, [vp, vp, vp, u64, vp])
    _decl(lib, "fs_read_quiet_orbit", u32, [vp, C.c_int, vp, u64, vp])
    _decl(lib, "fs_build_la", u32, [vp, C.c_int, vp, C.c_int])
    _decl(lib, "fs_build_la_mt", u32, [vp, C.c_int, vp, C.c_int, C.c_int])
    _decl(lib, "fs_la_counts", u32, [vp, vp, vp, vp, vp])
    _decl(lib, "fs_read_la", u32, [vp, vp, u32, vp, u32, vp])
    _decl(lib, "fs_group_create", vp, [vp, C.c_int, C.c_int])
    _decl(lib, "fs_group_destroy", None, [vp])
    _decl(lib, "fs_group_size", C.c_int, [vp])
    _decl(lib, "fs_group_transport", C.c_int, [vp])
    _decl(lib, "fs_group_renderer", vp, [vp, C.c_int])
    _decl(lib, "fs_group_init_memory", u32, [vp, u32, u32, u32, u32, vp, u32, u32, u64])
    _decl(lib, "fs_group_upload_orbit", u32, [vp, u64, C.c_int, u32, vp, u64, u64, u64])
    _decl(lib, "fs_group_upload_orbit_compressed", u32, [vp, u64, C.c_int, u32, vp, u64, u64, u64, vp, vp])
    _decl(lib, "fs_group_upload_la", u32, [vp, u64, C.c_int, u32, vp, u32, vp, u32, C.c_int, C.c_int, vp])
    _decl(lib, "fs_group_upload_bla", u32, [vp, C.c_int, vp, vp, i32, i32])
    _decl(lib, "fs_group_upload_orbit_scaled", u32, [vp, C.c_int, u32, vp, vp, u64, u64])
    _decl(lib, "fs_group_render_lav2", u32, [vp, C.c_int, C.c_int, C.c_int, vp, u64])
    _decl(lib, "fs_group_render_bla", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_group_render_scaled", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_group_render_direct", u32, [vp, C.c_int, vp, u64])
    _decl(lib, "fs_group_clear", u32, [vp])
    _decl(lib, "fs_group_render_current", u32, [vp, u64, vp, vp])
    _decl(lib, "fs_group_render_current_colors", u32, [vp, u64, vp, vp, vp, C.c_int])
    _decl(lib, "fs_group_sync_display", u32, [vp])
    _decl(lib, "fs_display_stream", vp, [vp])
    _decl(lib, "fs_colorize_frame", u32, [vp, vp, u64, vp, vp, vp])
    _decl(lib, "fs_color_buffer_elements", u64, [vp])
    _decl(lib, "fs_read_color_buffer", u32, [vp, vp])
    _decl(lib, "fs_group_sync", u32, [vp])
    _decl(lib, "fs_group_wait_current", u32, [vp, u32])
    _decl(lib, "fs_group_gather_ms", C.c_float, [vp])
    _decl(lib, "fs_group_plan", None, [u32, u32, u32, u32, vp, vp, vp])
    _decl(lib, "fs_group_set_host_path", u32, [vp, C.c_int])
    _decl(lib, "fs_group_host_path", C.c_int, [vp])
    _decl(lib, "fs_copy_bands_to_host", u32, [vp, vp, vp, vp])
    _decl(lib, "fs_host_register", u32, [vp, u64])
    _decl(lib, "fs_host_unregister", u32, [vp])
    _render = lib
    return lib


RENDER_SYMBOLS = [
    "fs_create", "fs_destroy", "fs_test_device_is_working", "fs_device_count", "fs_error_string", "fs_init_memory", "fs_set_row_bands",
    "fs_local_rows", "fs_set_external_iter_buffer", "fs_device_iter_buffer", "fs_rounded_width", "fs_upload_orbit", "fs_upload_orbit_compressed",
    "fs_upload_la", "fs_upload_bla", "fs_render_lav2", "fs_feature_eval", "fs_feature_eval_direct", "fs_set_feature_slice",
    "fs_feature_eval_resident", "fs_orbit_form", "fs_feature_eval_plain", "fs_feature_eval_plain_direct",
    "fs_autozoom_pick", "fs_set_autozoom_gather_cap",
    "fs_render_exact", "fs_exact_stable_mask", "fs_set_exact_slice", "fs_read_exact_stats",
    "fs_exact_sample_counts", "fs_exact_eval_points", "fs_exact_eval_points_wide", "fs_render_exact_wide", "fs_exact_wide_state", "fs_exact_audit",
    "fs_set_exact_cycle_check", "fs_read_exact_proved", "fs_read_exact_cycle_stats", "fs_set_exact_cycle_fingerprint_bits",
    "fs_set_exact_keep", "fs_render_exact_continue", "fs_exact_kept_info", "fs_exact_drop_kept",
    "fs_set_exact_periods", "fs_read_exact_atom_periods", "fs_read_exact_cycle_lengths", "fs_set_exact_atom_key_bits",
    "fs_render_bla", "fs_render_direct", "fs_upload_orbit_scaled",
    "fs_render_scaled", "fs_build_bla", "fs_bla_num_levels", "fs_bla_lm2", "fs_bla_level_size", "fs_read_bla_level",
    "fs_bla_lookup_probe", "fs_read_bla_native",
    "fs_render_direct_lp", "fs_clear",
    "fs_render_current", "fs_sync_compute", "fs_compute_stream", "fs_sync_display", "fs_query_compute", "fs_enqueue_done_callback",
    "fs_host_fallback_bytes", "fs_idle_device_bytes", "fs_release_idle_device_memory", "fs_set_compressed_orbit_mode", "fs_orbit_device_bytes", "fs_get_width", "fs_get_height", "fs_last_kernel_ms", "fs_set_kernel_variant", "fs_kernel_ms_history", "fs_kernel_ms_split_history", "fs_forget_tile_costs", "fs_last_frame_tile_ordered", "fs_last_frame_sampled_tile_order", "fs_read_tile_costs", "fs_read_tile_order", "fs_seq_cursor_probe", "fs_enable_step_count", "fs_read_step_count",
    "fs_time_render_current", "fs_read_stats_raw", "fs_test_block_threshold", "fs_test_ndz_threshold", "fs_read_ndz_bounds", "fs_read_quiet_orbit", "fs_build_la", "fs_build_la_mt", "fs_la_counts", "fs_read_la",
    "fs_group_create", "fs_group_destroy", "fs_group_size", "fs_group_transport", "fs_group_renderer", "fs_group_init_memory",
    "fs_group_upload_orbit", "fs_group_upload_orbit_compressed", "fs_group_upload_la", "fs_group_upload_bla",
    "fs_group_upload_orbit_scaled", "fs_group_render_lav2", "fs_group_render_bla", "fs_group_render_scaled",
    "fs_group_render_direct", "fs_group_clear", "fs_group_render_current", "fs_group_render_current_colors", "fs_group_sync_display", "fs_display_stream", "fs_colorize_frame",
    "fs_color_buffer_elements", "fs_read_color_buffer", "fs_group_sync", "fs_group_wait_current", "fs_group_gather_ms",
    "fs_group_plan", "fs_group_set_host_path", "fs_group_host_path", "fs_copy_bands_to_host", "fs_host_register", "fs_host_unregister",
]


def inputs_lib():
    """libfsinputs.so (GMP host builders)."""
    global _inputs
    if _inputs is not None:
        return _inputs
    path = _build.LIB_INPUTS
    if not os.path.exists(path):
        raise RuntimeError("libfsinputs.so is missing (%s): run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    _decl(lib, "fsh_view_create", vp, [C.c_char_p] * 4 + [u32, u32])
    _decl(lib, "fsh_view_destroy", None, [vp])
    _decl(lib, "fsh_view_autozoom_next", vp, [vp, C.c_double, C.c_double, u32, u32, u32])
    _decl(lib, "fsh_view_save_im", C.c_int, [vp, u64, C.c_char_p, C.c_int])
    _decl(lib, "fsh_view_load_im", vp, [C.c_char_p, u32, u32, C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(C.c_int)])
    _decl(lib, "fsh_view_precision_bits", u64, [vp])
    _decl(lib, "fsh_view_exact_axes", C.c_int, [vp, u32, u32, u32, C.c_int, u32, vp, vp])
    _decl(lib, "fsh_view_bbox_str", C.c_int, [vp, C.c_int, C.c_char_p, C.c_size_t])
    _decl(lib, "fsh_view_coords_direct_f64", None, [vp, u32, u32, vp])
    _decl(lib, "fsh_view_coords_direct_hdr32", None, [vp, u32, u32, vp])
    _decl(lib, "fsh_view_coords_direct_hdr64", None, [vp, u32, u32, vp])
    _decl(lib, "fsh_orbit_create", vp, [vp, C.c_int, u64, C.c_int])
    _decl(lib, "fsh_orbit_create_ex", vp, [vp, C.c_int, u64, C.c_int, C.c_int])
    _decl(lib, "fsh_orbit_is_compressed", C.c_int, [vp])
    _decl(lib, "fsh_orbit_compressed_count", u64, [vp])
    _decl(lib, "fsh_orbit_compressed_data_hdr32", vp, [vp])
    _decl(lib, "fsh_orbit_low_hdr32", None, [vp, vp])
    _decl(lib, "fsh_orbit_compressed_data_hdr64", vp, [vp])
    _decl(lib, "fsh_orbit_low_hdr64", None, [vp, vp])
    _decl(lib, "fsh_la_default_params", None, [C.POINTER(C.c_int32)])
    _decl(lib, "fsh_mpz_raw_write", C.c_size_t, [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t])
    _decl(lib, "fsh_mpz_raw_read", C.c_size_t, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t])
    _decl(lib, "fsh_orbit_save_im", C.c_int, [vp, u64, C.c_int, C.c_char_p, C.c_int])
    _decl(lib, "fsh_orbit_load_im", vp, [C.c_char_p, C.POINTER(u64)])
    _decl(lib, "fsh_orbit_is64", C.c_int, [vp])
    _decl(lib, "fsh_orbit_destroy", None, [vp])
    _decl(lib, "fsh_feature_begin", vp, [vp, vp, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_begin_direct", vp, [vp, C.c_int, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_begin_direct_at", vp, [vp, C.c_int, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_direct_grid", C.c_int, [vp, C.c_int, u32, u32, vp, vp])
    _decl(lib, "fsh_feature_pt_axes", C.c_int, [vp, vp, C.c_int, u32, u32, vp, vp, vp, vp, vp])
    _decl(lib, "fsh_feature_pt_grid", C.c_int, [vp, vp, C.c_int, u32, u32, vp, vp])
    _decl(lib, "fsh_feature_begin_plain", vp, [vp, vp, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_begin_plain_direct", vp, [vp, C.c_int, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_begin_plain_direct_at", vp, [vp, C.c_int, u32, u32, u32, u64])
    _decl(lib, "fsh_feature_plain_direct_grid", C.c_int, [vp, C.c_int, u32, u32, vp, vp])
    _decl(lib, "fsh_feature_kind", C.c_int, [vp])
    _decl(lib, "fsh_feature_destroy", None, [vp])
    _decl(lib, "fsh_feature_is64", C.c_int, [vp])
    _decl(lib, "fsh_feature_candidates", u64, [vp])
    _decl(lib, "fsh_feature_next_batch", u64, [vp, vp, u64, C.POINTER(C.c_int), vp, C.POINTER(u64)])
    _decl(lib, "fsh_feature_consume", None, [vp, vp, u64])
    _decl(lib, "fsh_feature_found", u64, [vp])
    _decl(lib, "fsh_feature_result", C.c_int, [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(u64),
                                                vp, C.POINTER(u32)])
    _decl(lib, "fsh_orbit_count", u64, [vp])
    _decl(lib, "fsh_orbit_scale_entries", u64, [vp, vp, vp, u64])
    _decl(lib, "fsh_orbit_scale_parts", u64, [vp, vp, vp, vp, u64])
    _decl(lib, "fsh_orbit_period", u64, [vp])
    _decl(lib, "fsh_orbit_data_hdr32", vp, [vp])
    _decl(lib, "fsh_orbit_data_hdr64", vp, [vp])
    _decl(lib, "fsh_orbit_max_radius_hdr32", None, [vp, vp])
    _decl(lib, "fsh_orbit_max_radius_hdr64", None, [vp, vp])
    _decl(lib, "fsh_orbit_data_hdr32_bad", vp, [vp])
    _decl(lib, "fsh_orbit_data_f32_bad", vp, [vp])
    _decl(lib, "fsh_orbit_bad_count", u64, [vp])
    _decl(lib, "fsh_view_coords_direct_lp", None, [vp, u32, u32, C.c_int, vp])
    _decl(lib, "fsh_view_coords_perturb_hdr32", None, [vp, vp, u32, u32, vp])
    _decl(lib, "fsh_view_coords_perturb_hdr64", None, [vp, vp, u32, u32, vp])
    _decl(lib, "fsh_df32_op", None, [C.c_int, vp, vp, vp])
    _decl(lib, "fsh_hr2_reduce", None, [vp])
    _decl(lib, "fsh_hr2_add", None, [vp, vp, C.c_int, vp])
    _decl(lib, "fsh_hc2_reduce", None, [vp])
    _decl(lib, "fsh_convert_orbit_hdr64_to_2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_convert_la_hdr64_to_2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_convert_at_hdr64_to_2x32", None, [vp, vp])
    _decl(lib, "fsh_view_coords_perturb_2x32", None, [vp, vp, u32, u32, vp])
    _decl(lib, "fsh_la_create_hdr32", vp, [vp, C.c_int])
    _decl(lib, "fsh_la_create", vp, [vp, C.c_int])
    _decl(lib, "fsh_la_create_ex", vp, [vp, C.c_int, C.c_int])
    _decl(lib, "fsh_la_is64", C.c_int, [vp])
    _decl(lib, "fsh_la_destroy", None, [vp])
    _decl(lib, "fsh_la_count", u32, [vp])
    _decl(lib, "fsh_la_data", vp, [vp])
    _decl(lib, "fsh_la_stage_count", u32, [vp])
    _decl(lib, "fsh_la_stages", vp, [vp])
    _decl(lib, "fsh_la_is_valid", C.c_int, [vp])
    _decl(lib, "fsh_la_use_at", C.c_int, [vp])
    _decl(lib, "fsh_la_at", None, [vp, vp])
    _decl(lib, "fsh_bla_create_hdr32", vp, [vp])
    _decl(lib, "fsh_bla_create", vp, [vp])
    _decl(lib, "fsh_bla_create_ex", vp, [vp, vp])
    _decl(lib, "fsh_bla_destroy", None, [vp])
    _decl(lib, "fsh_bla_num_levels", i32, [vp])
    _decl(lib, "fsh_bla_lm2", i32, [vp])
    _decl(lib, "fsh_bla_level_ptrs", vp, [vp])
    _decl(lib, "fsh_bla_level_sizes", vp, [vp])
    _decl(lib, "fsh_plain_create", vp, [vp, C.c_int, u64, C.c_int, C.c_int])
    _decl(lib, "fsh_plain_create_ex", vp, [vp, C.c_int, u64, C.c_int, C.c_int, C.c_int])
    _decl(lib, "fsh_plain_save_im", C.c_int, [vp, u64, C.c_int, C.c_char_p, C.c_int])
    _decl(lib, "fsh_plain_load_im", vp, [C.c_char_p, C.POINTER(u64), C.c_int])
    _decl(lib, "fsh_plain_is_compressed", C.c_int, [vp])
    _decl(lib, "fsh_plain_compressed_count", u64, [vp])
    _decl(lib, "fsh_plain_compressed_data", vp, [vp])
    _decl(lib, "fsh_plain_orbit_low", None, [vp, vp])
    _decl(lib, "fsh_convert_orbit_rc_f64_to_p2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_convert_orbit_rc_hdr64_to_2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_orbit_low_2x32", None, [vp, vp])
    _decl(lib, "fsh_plain_destroy", None, [vp])
    _decl(lib, "fsh_plain_kind", C.c_int, [vp])
    _decl(lib, "fsh_plain_orbit_count", u64, [vp])
    _decl(lib, "fsh_plain_orbit_period", u64, [vp])
    _decl(lib, "fsh_plain_orbit_data", vp, [vp])
    _decl(lib, "fsh_plain_la_count", u32, [vp])
    _decl(lib, "fsh_plain_la_data", vp, [vp])
    _decl(lib, "fsh_plain_la_stage_count", u32, [vp])
    _decl(lib, "fsh_plain_la_stages", vp, [vp])
    _decl(lib, "fsh_plain_la_is_valid", C.c_int, [vp])
    _decl(lib, "fsh_plain_la_use_at", C.c_int, [vp])
    _decl(lib, "fsh_plain_la_at", None, [vp, vp])
    _decl(lib, "fsh_plain_coords", None, [vp, vp, u32, u32, vp])
    _decl(lib, "fsh_convert_orbit_f64_to_p2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_convert_la_f64_to_p2x32", None, [vp, u64, vp])
    _decl(lib, "fsh_convert_at_f64_to_p2x32", None, [vp, vp])
    _decl(lib, "fsh_convert_coords_f64_to_p2x32", None, [vp, vp])
    _decl(lib, "fsh_orbit_f64_create", vp, [vp, u64, C.c_int])
    _decl(lib, "fsh_orbit_f64_destroy", None, [vp])
    _decl(lib, "fsh_orbit_f64_count", u64, [vp])
    _decl(lib, "fsh_orbit_f64_period", u64, [vp])
    _decl(lib, "fsh_orbit_f64_data", vp, [vp])
    _decl(lib, "fsh_orbit_f64_data_bad", vp, [vp])
    _decl(lib, "fsh_orbit_f64_data_f32_bad", vp, [vp])
    _decl(lib, "fsh_orbit_f64_bla_num_levels", i32, [vp])
    _decl(lib, "fsh_orbit_f64_bla_lm2", i32, [vp])
    _decl(lib, "fsh_orbit_f64_bla_level_ptrs", vp, [vp])
    _decl(lib, "fsh_orbit_f64_bla_level_sizes", vp, [vp])
    _decl(lib, "fsh_view_coords_perturb_f64", None, [vp, vp, u32, u32, vp])
    _inputs = lib
    return lib
