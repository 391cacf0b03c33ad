"""ctypes binding of the C-ABI in include/crfp_hip.h (libcrfp_hip.so, built in-tree by
``crfp_amd/csrc/Makefile``).  There is no fallback: if the library is missing every op raises."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRFP_HIP_LIB points at an alternative build of the same C-ABI (diagnostic variants); default: the in-tree build
LIB_PATH = os.environ.get("CRFP_HIP_LIB") or os.path.join(_HERE, "libcrfp_hip.so")

NUM_PARAMS = 118
RT_NUM_PARAMS = 158   # CRFP_RT_NUM_PARAMS
DSV_Y_ONLY, DSV_STRICT_F32, DSV_SINGLE_STREAM = 1, 2, 4   # flags of crfp_dsv_forward_clip / crfp_dsv_stream_frame
DSV_INPUTS_RESIDENT = 8   # crfp_dsv_stream_frame only
METRICS_LUMA = 1   # flag of crfp_frame_metrics_f32
GAZE_ROW_INTS, GAZE_EXISTS, GAZE_COUNTS = 24, 1, 2   # row length and entry flags of crfp_gaze_prep_f32
IO_BGR, IO_RECT_INTS, IO_HAS_FOVEA = 1, 4, 1   # call flag, row length and row flag of crfp_frame_ingest_u8 / crfp_frame_export_u8
IO_OUT_F32, IO_TWO_PASS = 2, 4   # flags of crfp_resize_bicubic_u8: fp32 planar output; the two-pass path whatever the geometry

c_float_p = C.POINTER(C.c_float)


class ProbeConv(C.Structure):
    """crfp_probe_conv of include/crfp_hip.h: one conv of a crfp_conv_probe call (test hook)."""
    _fields_ = [("src", C.c_void_p * 4), ("weight", C.c_void_p), ("bias", C.c_void_p), ("weight2", C.c_void_p), ("bias2", C.c_void_p),
                ("residual", C.c_void_p), ("flow", C.c_void_p), ("dst", C.c_void_p * 3), ("dst_raw", C.c_void_p * 3),
                ("nsrc", C.c_int), ("src_kind", C.c_int * 4), ("src_nch", C.c_int * 4), ("src_pad", C.c_int * 4),
                ("cout", C.c_int), ("cout_split", C.c_int), ("store", C.c_int), ("ps_r", C.c_int), ("act", C.c_int), ("n_off_quads", C.c_int),
                ("ndst", C.c_int), ("dst_q0", C.c_int * 3), ("dst_q1", C.c_int * 3), ("dst_pad", C.c_int * 3),
                ("strict", C.c_int), ("dst_f32", C.c_int), ("post_scale", C.c_float)]


class NarrowStencil(C.Structure):
    """crfp_narrow_stencil of include/crfp_hip.h: one stencil of a crfp_narrow_probe call (test hook)."""
    _fields_ = [("src", C.c_void_p * 3), ("weight", C.c_void_p), ("bias", C.c_void_p), ("weight2", C.c_void_p), ("bias2", C.c_void_p),
                ("residual", C.c_void_p), ("flow", C.c_void_p), ("base_lr", C.c_void_p), ("mask", C.c_void_p),
                ("dst", C.c_void_p), ("dst_raw", C.c_void_p), ("dst2", C.c_void_p), ("dst2_raw", C.c_void_p),
                ("nsrc", C.c_int), ("src_kind", C.c_int * 3), ("src_nch", C.c_int * 3), ("src_pad", C.c_int), ("dst_pad", C.c_int),
                ("cout", C.c_int), ("cout_split", C.c_int), ("act", C.c_int), ("epi", C.c_int), ("y_only", C.c_int), ("gate_h", C.c_int),
                ("dst2_on", C.c_int), ("post_scale", C.c_float)]


class NarrowReport(C.Structure):
    """crfp_narrow_report: the kernel a narrow launch took, its template arguments, its tiles and workgroups per batch item."""
    _fields_ = [(k, C.c_int) for k in ("kernel", "kq", "epi", "gate", "st2", "kqg", "res", "tiles", "workgroups")]


class DcnTailArgs(C.Structure):
    """crfp_dcn_tail_args of include/crfp_hip.h: the device buffers of a crfp_dcn_tail_probe call (test hook)."""
    _fields_ = [(k, C.c_void_p) for k in ("feat", "flow", "wconv", "bconv", "x", "wdcn", "bdcn", "out", "status", "warp_src", "warp_flow", "warp_dst")] + \
               [(k, C.c_longlong) for k in ("feat_b", "flow_b", "x_b", "out_b", "warp_src_b", "warp_flow_b", "warp_dst_b")] + \
               [(k, C.c_int) for k in ("n", "h", "w", "bands")]


class DcnTailReport(C.Structure):
    """crfp_dcn_tail_report: how the fused DCN launch of a crfp_dcn_tail_probe call is sized."""
    _fields_ = [(k, C.c_int) for k in ("cus", "tiles", "persistent", "warp_wgs", "plan_taken", "grid")]


class GatherArgs(C.Structure):
    """crfp_gather_args of include/crfp_hip.h: the NCHW fp32 tensors and the mode of a crfp_gather_probe call (test hook)."""
    _fields_ = [(k, C.c_void_p) for k in ("x", "x2", "aux", "mask", "flow", "head_w", "head_b", "weight", "bias", "out", "out2", "out_raw", "out2_raw",
                                          "status")] + [(k, C.c_int) for k in ("mode", "c", "n", "h", "w")]


class GatherReport(C.Structure):
    """crfp_gather_report: the kernel a gather launch took, how a fused DCN launch is sized, the strides of the raw destinations."""
    _fields_ = [(k, C.c_int) for k in ("kernel", "cus", "tiles", "persistent", "split", "rsv")] + [(k, C.c_longlong) for k in ("out_stride", "out2_stride")]


GATHER_MODES = {"warp": 0, "warp_dual": 1, "dcn_g8": 2, "dcn_fused": 3, "dcn3": 4, "dcn3_fused": 5}   # CRFP_GPROBE_*
GATHER_KERNELS = ("none", "flow_warp_p4", "flow_warp_p4_dual_split", "flow_warp_p4_dual", "dcn_g8_pipe", "dcn_fused", "dcn_fused_persistent", "dcn3",
                  "dcn3_fused")   # CRFP_GATHERK_*
NARROW_KERNELS = ("none", "narrow", "seq", "pair", "chain")   # CRFP_NARROWK_*
NARROW_MODES = {"single": 0, "pair": 1, "chain": 2}
NARROW_EPI = {"plain": 0, "blend": 1, "last": 2, "offmask3": 3}
_NARROW_HEAD = [C.c_int] + [C.POINTER(NarrowStencil)] * 3 + [C.c_int] * 4

# kernel variants crfp_conv_probe reports (CRFP_CONVK_*)
CONV_KERNELS = ("none", "mfma_shift_ct2", "mfma_shift", "mfma_ct2", "mfma_rows4", "mfma_rows8", "split8", "split4", "split_dual", "bf16_x8",
                "bf16_4w", "bf16_pair", "split_pair")
PROBE_MODES = {"single": 0, "dual": 1, "pair": 2, "s3_chain": 3, "pair_f32": 4}
PROBE_SRC = {"q4": 0, "unshuf4": 2, "flow2": 3}
PROBE_STORE = {"q4": 0, "ps": 1, "offmask": 3}


class ProfRecord(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int), ("total_ms", C.c_double),
                ("bytes", C.c_double), ("flops", C.c_double)]


# name -> (restype, argtypes); mirrors include/crfp_hip.h one to one
SIGNATURES = {
    "crfp_version": (C.c_int, []),
    "crfp_last_error_string": (C.c_char_p, []),
    "crfp_shutdown": (C.c_int, []),
    "crfp_flow_warp_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_flow_warp_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dcnv2_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "crfp_dcnv2_forward_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dcnv2_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "crfp_dcnv2_backward_f32": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dcnv2_shared_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_dcnv2_shared_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dcnv2_shared_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_dcnv2_shared_backward_f32": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_flow_warp_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_flow_warp_backward_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_flow_warp_backward_window_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_conv3x3_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "crfp_conv3x3_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_conv3x3_ex_workspace_bytes": (C.c_size_t, [C.c_int] * 9),
    "crfp_conv3x3_ex_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float] + [C.c_int] * 4 +
                            [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_conv3x3_ex_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 8),
    "crfp_conv3x3_ex_backward_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_float] +
                                     [C.c_int] * 2 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_conv3x3_packed_bytes": (C.c_size_t, [C.c_int] * 2),
    "crfp_conv3x3_pack_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_conv3x3_packed_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float, C.c_void_p]),
    "crfp_dcnv2_g8_packed_bytes": (C.c_size_t, []),
    "crfp_dcnv2_g8_pack_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_size_t, C.c_void_p]),
    "crfp_dcnv2_g8_packed_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_upsample_bilinear_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_float] * 3 + [C.c_void_p]),
    "crfp_upsample_bilinear_ac_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_float, C.c_void_p]),
    "crfp_convkxk_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p]),
    "crfp_spynet_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "crfp_spynet_forward": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_psnr_partial_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "crfp_avgpool2_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "crfp_upsample_bilinear_backward_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_float] * 3 + [C.c_void_p]),
    "crfp_avgpool2_backward_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "crfp_charbonnier_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_charbonnier_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_charbonnier_backward_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "crfp_fovea_head_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "crfp_fovea_head_f32": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_psnr_ssim_partial_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] * 2 + [C.c_void_p]),
    "crfp_window_scores_workspace_bytes": (C.c_size_t, [C.c_int]),
    "crfp_window_scores_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_frame_metrics_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_frame_metrics_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_gaze_prep_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p]),
    "crfp_frame_ingest_u8": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_void_p]),
    "crfp_frame_export_u8": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]),
    "crfp_bicubic_taps": (C.c_int, [C.c_int] * 2 + [C.POINTER(C.c_int32)] * 2 + [C.c_int]),
    "crfp_resize_bicubic_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "crfp_resize_bicubic_u8": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_frame_export_y_bicubic_u8": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_param_name": (C.c_char_p, [C.c_int]),
    "crfp_dsv_param_numel": (C.c_int, [C.c_int, C.c_int]),
    "crfp_dsv_packed_weight_bytes": (C.c_size_t, [C.c_int]),
    "crfp_dsv_pack_weights": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "crfp_dsv_status_offset": (C.c_size_t, [C.c_int] * 3),
    "crfp_dsv_forward_clip": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 +
                              [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_batch_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "crfp_dsv_batch_status_offset": (C.c_size_t, [C.c_int] * 4),
    "crfp_dsv_forward_batch": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 4 +
                               [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_stream_frame": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 3 +
                              [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_stream_batch": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 4 +
                              [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_fnet_forward": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_rt_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "crfp_rt_forward_clip": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_rt_debug_fetch": (C.c_int, [C.c_char_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p] + [C.POINTER(C.c_int)] * 3 + [C.c_void_p]),
    "crfp_prof_enable": (C.c_int, [C.c_int]),
    "crfp_prof_reset": (C.c_int, []),
    "crfp_debug_side_tables": (C.c_int, []),
    "crfp_prof_report": (C.c_int, [C.POINTER(ProfRecord), C.c_int]),
    "crfp_conv_probe_workspace_bytes": (C.c_size_t, [C.c_int, C.POINTER(ProbeConv), C.POINTER(ProbeConv)] + [C.c_int] * 3),
    "crfp_conv_probe_kernel": (C.c_int, [C.c_int, C.POINTER(ProbeConv), C.POINTER(ProbeConv)] + [C.c_int] * 3 + [C.POINTER(C.c_int)]),
    "crfp_conv_probe": (C.c_int, [C.c_int, C.POINTER(ProbeConv), C.POINTER(ProbeConv)] + [C.c_int] * 3 + [C.c_void_p, C.POINTER(C.c_int)] +
                        [C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_narrow_probe_workspace_bytes": (C.c_size_t, _NARROW_HEAD),
    "crfp_narrow_probe_plan": (C.c_int, _NARROW_HEAD + [C.POINTER(NarrowReport)]),
    "crfp_narrow_probe": (C.c_int, _NARROW_HEAD + [C.c_void_p, C.c_void_p, C.POINTER(NarrowReport), C.c_void_p, C.c_size_t, C.c_void_p]),
    "crfp_dsv_debug_fetch": (C.c_int, [C.c_char_p] + [C.c_int] * 3 + [C.c_void_p, C.c_void_p] +
                             [C.POINTER(C.c_int)] * 3 + [C.c_void_p]),
    "crfp_dcn_tail_plan": (C.c_int, [C.POINTER(DcnTailArgs), C.POINTER(DcnTailReport)]),
    "crfp_dcn_tail_probe": (C.c_int, [C.POINTER(DcnTailArgs), C.POINTER(DcnTailReport), C.c_void_p]),
    "crfp_gather_probe_workspace_bytes": (C.c_size_t, [C.POINTER(GatherArgs)]),
    "crfp_gather_probe_plan": (C.c_int, [C.POINTER(GatherArgs), C.POINTER(GatherReport)]),
    "crfp_gather_probe": (C.c_int, [C.POINTER(GatherArgs), C.POINTER(GatherReport), C.c_void_p, C.c_size_t, C.c_void_p]),
}
CRA_NUM_PARAMS = 144


@dataclasses.dataclass(frozen=True)
class Family:
    """One engine family of the C-ABI: what crfp_amd.engine's handles and the bindings below know about a wiring."""
    prefix: str          # C-ABI prefix of its entry points
    names: str           # the family whose param_name table (and parameter count) names its parameters
    num_params: int
    model: str           # the model class, for error messages
    ops: frozenset       # the operations it exports, as `prefix + op`
    bf16: frozenset      # those with a bf16-storage twin `prefix + op + "_bf16"` (same argument list)


_PACK = frozenset(("param_numel", "packed_weight_bytes", "pack_weights"))
_CLIP = _PACK | {"batch_workspace_bytes", "batch_status_offset", "forward_batch"}   # clip / lock-step batch forward
_STREAM = _CLIP | {"stream_batch"}                                                  # + one frame per call
_FETCH = _STREAM | {"debug_fetch"}                                                  # + the workspace fetch of the wiring's own Layout
_DSV = _FETCH | {"fnet_forward"}
_NUMEL = frozenset(("param_numel",))   # shapes do not depend on the storage type
# dsv: CRFP_DSV.  cra: CRFP_DSV_CRA, its own parameter table, clip forward and the one-frame-per-call form (MRCF_simple_v18_cra).  simple /
# dense: the CRFP_simple / CRFP wirings -- CRFP_DSV's parameter names with their own shapes -- clip forward and the one-frame-per-call form
# (MRCF_simple_v13 / v15).  rt: the regional benchmark wiring, fp32 storage only, with a forward call, a workspace query and a debug fetch of its own.
FAMILIES = {
    "dsv": Family("crfp_dsv_", "dsv", NUM_PARAMS, "CRFP_DSV", _DSV, _DSV - _NUMEL),
    "cra": Family("crfp_cra_", "cra", CRA_NUM_PARAMS, "CRFP_DSV_CRA", _FETCH, _FETCH - _NUMEL),
    "simple": Family("crfp_simple_", "dsv", NUM_PARAMS, "CRFP_simple", _FETCH, _FETCH - _NUMEL),
    "dense": Family("crfp_dense_", "dsv", NUM_PARAMS, "CRFP", _FETCH, _FETCH - _NUMEL),
    "rt": Family("crfp_rt_", "rt", RT_NUM_PARAMS, "MRCF_simple_v18", _PACK | {"workspace_bytes", "forward_clip", "debug_fetch"}, frozenset()),
}


def symbol(family: str, op: str, storage: str = "f32") -> str:
    """The C name of operation `op` for a family and a storage type.  NotImplementedError when the family does not export it."""
    row = FAMILIES[family]
    if op not in row.ops:
        raise NotImplementedError(f"crfp_amd: {row.model} has no {op} entry point")
    base = "crfp_fnet_forward" if op == "fnet_forward" else row.prefix + op   # the flow network alone carries no family prefix
    return base + ("_bf16" if storage == "bf16" and op in row.bf16 else "")


# per-family entries: a name that is not spelled out above has the argument list of CRFP_DSV's entry point for the same operation
for _k, _row in FAMILIES.items():
    SIGNATURES.setdefault(FAMILIES[_row.names].prefix + "param_name", SIGNATURES["crfp_dsv_param_name"])
    for _op in _row.ops:
        for _st in ("f32", "bf16"):
            if symbol(_k, _op, _st) not in SIGNATURES:
                SIGNATURES[symbol(_k, _op, _st)] = SIGNATURES[symbol("dsv", _op)]
# bf16-storage twins of the C-ABI's n = 1 conveniences (crfp_dsv_forward_clip = crfp_dsv_forward_batch with n = 1, and so on)
for _n in ("workspace_bytes", "status_offset", "forward_clip", "stream_frame"):
    SIGNATURES[f"crfp_dsv_{_n}_bf16"] = SIGNATURES[f"crfp_dsv_{_n}"]

for _n in ("workspace_bytes", "kernel", ""):
    _n = "crfp_conv_probe" + ("_" + _n if _n else "")
    SIGNATURES[_n + "_bf16"] = SIGNATURES[_n]
for _n in ("workspace_bytes", "plan", ""):
    _n = "crfp_narrow_probe" + ("_" + _n if _n else "")
    SIGNATURES[_n + "_bf16"] = SIGNATURES[_n]
for _n in ("crfp_dcn_tail_plan", "crfp_dcn_tail_probe", "crfp_gather_probe_workspace_bytes", "crfp_gather_probe_plan", "crfp_gather_probe"):
    SIGNATURES[_n + "_bf16"] = SIGNATURES[_n]

_lib = None


def lib():
    """Load libcrfp_hip.so (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C crfp_amd/csrc`. "
                "crfp_amd has no CPU or PyTorch fallback path.")
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Import torch first so
        # that ONE HIP runtime serves both torch and this library (streams and device pointers are
        # shared across the C-ABI); loading in the other order leaves the process with a runtime
        # torch's bundled HSA stack cannot drive ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def kernel_source_digest() -> str:
    """sha256 (12 hex digits) over the kernel sources (csrc/*.hip, *.h, *.inc, Makefile): names the build a profile was taken with, so that
    bench.py can tell when the committed PMC summary belongs to other kernels than the ones it is timing (`stale`)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(_HERE, "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.inc")) + [os.path.join(d, "Makefile")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().crfp_last_error_string().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def prof_report(cap: int = 256):
    arr = (ProfRecord * cap)()
    n = lib().crfp_prof_report(arr, cap)
    return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                 bytes=arr[i].bytes, flops=arr[i].flops) for i in range(min(n, cap))]
