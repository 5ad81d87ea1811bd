"""ctypes binding of libdowngan_hip.so (the C ABI declared in include/downgan_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C downgan_amd/csrc``.
There is no fallback: if the shared object is missing, loading raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DG_LIB_OVERRIDE") or os.path.join(_HERE, "csrc", "libdowngan_hip.so")   # override: A/B builds in tools/

DG_F32, DG_BF16 = 0, 1
STATUS = {0: "DG_OK", -1: "DG_ERR_BAD_SHAPE", -2: "DG_ERR_BAD_DTYPE", -3: "DG_ERR_BAD_ARG", -4: "DG_ERR_LAUNCH"}


class Epilogue(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("has_act", C.c_int), ("act_slope", C.c_float),
                ("r1", C.c_void_p), ("ldr1", C.c_int64), ("s1", C.c_float),
                ("r2", C.c_void_p), ("ldr2", C.c_int64), ("s2", C.c_float),
                ("mask", C.c_void_p), ("ldmask", C.c_int64), ("mask_slope", C.c_float),
                ("accumulate", C.c_int), ("mask_bits", C.c_void_p), ("out_bits", C.c_void_p),
                ("mask_c0", C.c_int), ("mask_last", C.c_int), ("out_q", C.c_void_p), ("out_qs", C.c_void_p), ("ldqs", C.c_int64),
                ("out_u", C.c_void_p), ("out_ue", C.c_void_p), ("skip_y", C.c_int), ("out_amax", C.c_void_p)]


class ConvGeom(C.Structure):
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("Cin", C.c_int), ("Cout", C.c_int), ("stride", C.c_int), ("cin_real", C.c_int), ("pixel_shuffle", C.c_int),
                ("ldx", C.c_int64), ("ldy", C.c_int64)]


class GGDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("Hs", C.c_int), ("Ws", C.c_int), ("Cred", C.c_int),
                ("lds", C.c_int64), ("src_ps", C.c_int),
                ("Hg", C.c_int), ("Wg", C.c_int), ("sy_mul", C.c_int), ("sx_mul", C.c_int),
                ("ntaps", C.c_int), ("tap_dy", C.c_int * 9), ("tap_dx", C.c_int * 9), ("tap_w", C.c_int * 9),
                ("Nout", C.c_int), ("ldw", C.c_int64),
                ("Hd", C.c_int), ("Wd", C.c_int), ("ldd", C.c_int64),
                ("dy_mul", C.c_int), ("dx_mul", C.c_int), ("dy_off", C.c_int), ("dx_off", C.c_int),
                ("dst_ps", C.c_int)]


class SsimParams(C.Structure):
    _fields_ = [("win", C.c_int), ("g", C.c_float * 11), ("C1", C.c_float), ("C2", C.c_float)]


class MsssimCombine(C.Structure):
    _fields_ = [("inv_count", C.c_float * 5), ("weight", C.c_float * 5)]


class F8Operands(C.Structure):
    _fields_ = [("xq", C.c_void_p), ("xs", C.c_void_p), ("ldxq", C.c_int64), ("ldxs", C.c_int64), ("wq", C.c_void_p), ("ws", C.c_void_p)]


MAX_FIELDS = 8


class FieldPlanes(C.Structure):
    _fields_ = [("plane", C.c_void_p * MAX_FIELDS), ("mean", C.c_float * MAX_FIELDS), ("inv_std", C.c_float * MAX_FIELDS), ("c", C.c_int)]


EXP_BATCH_MAX = 16


class ExpBatch(C.Structure):
    _fields_ = [("scales", C.c_void_p * EXP_BATCH_MAX), ("rows", C.c_int64 * EXP_BATCH_MAX), ("ld", C.c_int64 * EXP_BATCH_MAX),
                ("nblocks", C.c_int * EXP_BATCH_MAX), ("out", C.c_void_p * EXP_BATCH_MAX), ("n", C.c_int)]


FINITE_MAX = 8


class FiniteBufs(C.Structure):
    _fields_ = [("ptr", C.c_void_p * FINITE_MAX), ("n", C.c_int64 * FINITE_MAX), ("dtype", C.c_int * FINITE_MAX), ("nbuf", C.c_int)]


EOF_MAX_C, EOF_MAX_K = 8, 64
RAPSD_MAX_N = 2048
HIST_MAX_BINS, HIST_MAX_OUT = 4096, EOF_MAX_C + 1
GRID_MAX_THR = 4
FSS_MAX_THR, FSS_MAX_SCALES, FSS_MAX_SIDE = 4, 8, 2048
ISCALE_MAX_THR, ISCALE_MAX_LEVELS, ISCALE_MAX_SIDE = 4, 12, 2048
DEFORM_MAX_LEVELS, DEFORM_MAX_SIDE, DEFORM_SCALARS = 4, 2048, 5
HIST2D_MAX_PAIRS, HIST2D_MAX_CELLS, HIST2D_MAX_SECTORS = 8, 16384, 72
INCR_MAX_LAGS, INCR_MAX_LAG, INCR_MAX_BINS, INCR_MAX_SIDE = 8, 256, 512, 2048
GRIDHIST_MAX_BINS, GRIDHIST_MAX_Q = 256, 16
OBJ_MAX_SIDE, OBJ_MAX_THR, OBJ_COLS = 2048, 4, 12
DIST_MAX_SIDE, DIST_MAX_THR, DIST_MAX_RINGS, DIST_MAX_CUTOFF, DIST_COLS, DIST_FAR = 2048, 4, 128, 512, 11, 1 << 30
TEMPORAL_MAX_THR, TEMPORAL_MAX_DUR, TEMPORAL_MAX_LAGS, TEMPORAL_MAX_LAG, TEMPORAL_MAX_BINS = 4, 256, 4, 24, 512


class EofFields(C.Structure):
    _fields_ = [("base", C.c_void_p), ("dtype", C.c_int), ("T", C.c_int), ("C", C.c_int), ("P", C.c_int),
                ("ld_t", C.c_int64), ("ld_c", C.c_int64), ("ld_p", C.c_int64)]


class HistSpec(C.Structure):
    _fields_ = [("nbins", C.c_int), ("speed_u", C.c_int), ("speed_v", C.c_int), ("lo", C.c_float * HIST_MAX_OUT),
                ("inv_w", C.c_float * HIST_MAX_OUT), ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C)]


class GridSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("scale", C.c_float * EOF_MAX_C),
                ("offset", C.c_float * EOF_MAX_C), ("pivot", C.c_float * HIST_MAX_OUT),
                ("thr", (C.c_float * GRID_MAX_THR) * HIST_MAX_OUT)]


class FssSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("nscale", C.c_int),
                ("win", C.c_int * FSS_MAX_SCALES), ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C),
                ("thr", (C.c_float * FSS_MAX_THR) * HIST_MAX_OUT)]


class IscaleSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("scale", C.c_float * EOF_MAX_C),
                ("offset", C.c_float * EOF_MAX_C), ("thr", (C.c_float * ISCALE_MAX_THR) * HIST_MAX_OUT)]


class DeformSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("levels", C.c_int), ("scale", C.c_float * EOF_MAX_C),
                ("offset", C.c_float * EOF_MAX_C), ("lo", C.c_float * HIST_MAX_OUT), ("inv_step", C.c_float * HIST_MAX_OUT)]


class Hist2dAxis(C.Structure):
    _fields_ = [("src", C.c_int), ("chan", C.c_int), ("nbins", C.c_int), ("lo", C.c_float), ("inv_w", C.c_float)]


class Hist2dSpec(C.Structure):
    _fields_ = [("npairs", C.c_int), ("speed_u", C.c_int), ("speed_v", C.c_int), ("nsec", C.c_int), ("calm", C.c_float),
                ("tan_k", C.c_float * (HIST2D_MAX_SECTORS // 4)), ("scale", C.c_float * EOF_MAX_C),
                ("offset", C.c_float * EOF_MAX_C), ("ax", (Hist2dAxis * 2) * HIST2D_MAX_PAIRS)]


class IncrSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nlag", C.c_int), ("nbins", C.c_int),
                ("lag", C.c_int * INCR_MAX_LAGS), ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C),
                ("lo", (C.c_float * INCR_MAX_LAGS) * HIST_MAX_OUT), ("inv_w", (C.c_float * INCR_MAX_LAGS) * HIST_MAX_OUT)]


class ObjectsSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("connectivity", C.c_int),
                ("inv_quantum", C.c_float), ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C),
                ("thr", (C.c_float * OBJ_MAX_THR) * HIST_MAX_OUT)]


class DistmapSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("nring", C.c_int), ("cutoff", C.c_int),
                ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C),
                ("thr", (C.c_float * DIST_MAX_THR) * HIST_MAX_OUT)]


class TemporalSpec(C.Structure):
    _fields_ = [("speed_u", C.c_int), ("speed_v", C.c_int), ("nthr", C.c_int), ("ndur", C.c_int), ("nlag", C.c_int),
                ("nbins", C.c_int), ("below", C.c_int * TEMPORAL_MAX_THR), ("lag", C.c_int * TEMPORAL_MAX_LAGS),
                ("scale", C.c_float * EOF_MAX_C), ("offset", C.c_float * EOF_MAX_C),
                ("thr", (C.c_float * TEMPORAL_MAX_THR) * HIST_MAX_OUT), ("lo", (C.c_float * TEMPORAL_MAX_LAGS) * HIST_MAX_OUT),
                ("inv_w", (C.c_float * TEMPORAL_MAX_LAGS) * HIST_MAX_OUT)]


MINMAX_PARTS = 256
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_PROTOS = {
    "dg_conv3x3_fwd": [C.POINTER(ConvGeom), C.POINTER(Epilogue), _vp, _vp, _vp, _vp],
    "dg_conv3x3_dgrad": [C.POINTER(ConvGeom), C.POINTER(Epilogue), _vp, _vp, _vp, _vp],
    "dg_conv3x3_wgrad": [C.POINTER(ConvGeom), _vp, _vp, _vp, _vp, _vp],
    "dg_conv3x3_wgrad_dense": [_vp, _i, _vp, _vp, _vp, _vp, _vp],
    "dg_conv3x3_wgrad_f8": [C.POINTER(ConvGeom), _vp, _vp, _vp, _vp, _vp, _vp],
    "dg_exp_from_amax": [_vp, _i, _i, _vp, _vp],
    "dg_conv3x3_wgrad_dense_f8": [C.POINTER(ConvGeom), _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "dg_gather_gemm": [C.POINTER(GGDesc), C.POINTER(Epilogue), _vp, _vp, _vp, _vp],
    "dg_conv3x3_plan": [C.POINTER(ConvGeom), _i, C.POINTER(GGDesc)],
    "dg_last_conv_kernels": [],
    "dg_last_wgrad_kernel": [],
    "dg_conv3x3_dgrad_launches": [C.POINTER(ConvGeom)],
    "dg_conv3x3_dgrad_stream_eligible": [C.POINTER(ConvGeom), C.POINTER(Epilogue)],
    "dg_set_s2_dgrad_stream": [C.c_int],
    "dg_colsum": [_i, _vp, _i64, _i64, _i64, _i64, _i, _vp, _vp],
    "dg_colsum_multi": [_i, _vp, _i64, _i64, _i, _i, _vp, _vp],
    "dg_repack_conv_weights": [_i, _i, _vp, _vp, _i, _i, _vp],
    "dg_repack_dense_dgrad": [_i, _vp, _i, _i, _vp, _vp],
    "dg_wgrad_unswap": [_vp, _vp, _i, _i, _vp],
    "dg_linear_fwd": [_i, _vp, _i64, _vp, _i64, _vp, _i, _i, _i, _i64, _vp],
    "dg_linear_dx": [_i, _i, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, _i, _i, _i64, _vp],
    "dg_linear_dw": [_i, _vp, _i, _vp, _i64, _vp, _i64, _i, _i, _i64, _vp],
    "dg_linear_dw_wide": [_i, _vp, _i, _vp, _i64, _vp, _i64, _i, _i, _i64, _i, _vp],
    "dg_bias_act": [_i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _f, _vp],
    "dg_mask_mul": [_i, _vp, _i64, _vp, _i64, _i64, _i, _f, _vp],
    "dg_axpby": [_i, _vp, _i64, _vp, _i64, _f, _vp, _i64, _f, _i64, _i, _vp],
    "dg_gp_interp": [_i, _vp, _vp, _vp, _vp, _i, _i64, _vp],
    "dg_gp_interp_c2": [_i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i, _i64, _vp],
    "dg_scale_rows_c2": [_i, _vp, _i64, _vp, _vp, _i, _i64, _vp],
    "dg_sumsq_rows": [_i, _vp, _i, _i64, _vp, _vp],
    "dg_gp_finish": [_vp, _i, _i, _f, _f, _vp, _vp, _vp],
    "dg_scale_rows": [_i, _vp, _vp, _vp, _i, _i64, _vp],
    "dg_l1": [_i, _vp, _i64, _vp, _i64, _i64, _i, _vp, _vp, _i64, _f, _vp, _i64, _vp],
    "dg_sqdiff": [_i, _vp, _i64, _vp, _i64, _i64, _i, _vp, _vp],
    "dg_sum_strided": [_vp, _i, _i, _f, _vp, _vp],
    "dg_fill_col": [_vp, _i, _i, _i, _f, _vp],
    "dg_adam": [_vp, _vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _i, _f, _vp],
    "dg_nchw_to_nhwc": [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "dg_nhwc_to_nchw": [_i, _vp, _i64, _vp, _i, _i, _i, _i, _vp],
    "dg_cast": [_i, _vp, _vp, _i64, _vp],
    "dg_minmax_partial": [_i, _vp, _i64, _i64, _i, _vp, _vp],
    "dg_minmax_finish": [_vp, _i, _vp, _vp],
    "dg_normalise_planar": [_i, _vp, _i, _i, _i, _i64, _i, _vp, _vp, _vp],
    "dg_ssim_level": [_vp, _vp, _i, _i, _i, C.POINTER(SsimParams), _vp, _vp],
    "dg_avgpool2": [_vp, _vp, _i, _i, _i, _vp],
    "dg_msssim_finish": [_vp, _i, _i, C.POINTER(MsssimCombine), _vp, _vp],
    "dg_div_vort_sums": [_i, _vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp],
    "dg_gather_samples": [_i, _vp, _i64, _i, _vp, _i, _vp, _i, _vp],
    "dg_quant_mxfp8": [_i, _vp, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp],
    "dg_block_exp_max": [_vp, _i64, _i64, _i, _i, _vp, _vp, _vp],
    "dg_block_exp_max_batch": [C.POINTER(ExpBatch), _i, _vp, _vp],
    "dg_quant_uniform": [_i, _vp, _i64, _i64, _i, _vp, _vp, _i64, _vp],
    "dg_conv3x3_fwd_f8": [C.POINTER(ConvGeom), C.POINTER(Epilogue), C.POINTER(F8Operands), _vp, _vp],
    "dg_conv3x3_dgrad_f8": [C.POINTER(ConvGeom), C.POINTER(Epilogue), C.POINTER(F8Operands), _vp, _vp],
    "dg_moments": [_vp, _i64, _vp, _vp],
    "dg_stage_fields": [_i, C.POINTER(FieldPlanes), _i64, _vp, _vp],
    "dg_lowpass5": [_i, _vp, _i64, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp],
    "dg_lowpass5_adjoint": [_i, _vp, _i64, _i, _i, _i, _i, _vp, _i64, _vp],
    "dg_set_deterministic_workspace": [_vp, _i64],
    "dg_deterministic": [],
    "dg_count_nonfinite": [C.POINTER(FiniteBufs), _vp, _vp],
    "dg_eof_mean": [C.POINTER(EofFields), _vp, _vp],
    "dg_eof_gram": [C.POINTER(EofFields), _vp, _i, _vp, _vp, _vp],
    "dg_eof_components": [C.POINTER(EofFields), _vp, _vp, _i, _vp, _i64, _i64, _vp, _vp],
    "dg_eof_flip": [_vp, _i, _i, _i, _i64, _i64, _vp, _vp],
    "dg_eof_project": [C.POINTER(EofFields), _vp, _vp, _i, _i64, _i64, _i, _vp, _vp, _vp],
    "dg_eof_reconstruct": [_vp, _i, _i, _i, _vp, _i64, _i64, _i, _vp, _vp, _vp],
    "dg_rapsd_ws_bytes": [_i, _i, _i],
    "dg_rapsd": [C.POINTER(EofFields), _i, _vp, _vp, _vp, _vp],
    "dg_rapsd_ring_counts": [_i, C.POINTER(_i64)],
    "dg_cross_rapsd_ws_bytes": [_i, _i, _i],
    "dg_cross_rapsd": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _vp, _vp, _vp, _vp],
    "dg_helmholtz_ws_bytes": [_i, _i],
    "dg_helmholtz": [C.POINTER(EofFields), _i, _i, C.POINTER(_f), _i, _vp, _vp, _vp, _vp],
    "dg_helmholtz_cross_ws_bytes": [_i, _i],
    "dg_helmholtz_cross": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(_f), _i, _vp, _vp, _vp, _vp],
    "dg_hist_ws_bytes": [C.POINTER(EofFields), C.POINTER(HistSpec)],
    "dg_hist": [C.POINTER(EofFields), C.POINTER(HistSpec), _vp, _vp, _vp, _vp, _vp],
    "dg_hist_host_bins": [C.POINTER(HistSpec), _vp, _i, _i64, _vp],
    "dg_gridstats_ws_bytes": [C.POINTER(EofFields), _i, C.POINTER(GridSpec)],
    "dg_gridstats_slices": [_i, _i],
    "dg_gridstats": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(GridSpec), _vp, _vp, _vp, _vp, _vp],
    "dg_fss_ws_bytes": [C.POINTER(EofFields), _i, _i, C.POINTER(FssSpec)],
    "dg_fss": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(FssSpec), _vp, _vp, _vp, _vp, _vp],
    "dg_fss_host": [C.POINTER(FssSpec), _vp, _vp, _i, _i, _i, _vp, _vp],
    "dg_fss_bound": [_i, _i, _i],
    "dg_iscale_levels": [_i, _i],
    "dg_iscale_bound": [_i, _i],
    "dg_iscale_ws_bytes": [C.POINTER(EofFields), _i, _i, C.POINTER(IscaleSpec)],
    "dg_iscale": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(IscaleSpec), _vp, _vp, _vp, _vp],
    "dg_iscale_host": [C.POINTER(IscaleSpec), _vp, _vp, _i, _i, _i, _vp],
    "dg_deform_bound": [_i, _i],
    "dg_deform_ws_bytes": [C.POINTER(EofFields), _i, _i, C.POINTER(DeformSpec)],
    "dg_deform": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(DeformSpec), _vp, _vp, _vp, _vp],
    "dg_deform_field": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(DeformSpec), _vp, _vp, _vp, _vp],
    "dg_deform_host": [C.POINTER(DeformSpec), _vp, _vp, _i, _i, _i, _vp, _vp],
    "dg_deform_field_host": [C.POINTER(DeformSpec), _vp, _vp, _i, _i, _i, _vp, _vp],
    "dg_hist2d_ws_bytes": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(Hist2dSpec)],
    "dg_hist2d": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(Hist2dSpec), _vp, _vp, _vp],
    "dg_hist2d_host_bins": [C.POINTER(Hist2dSpec), _vp, _vp, _i, _i64, _vp],
    "dg_incr_ws_bytes": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(IncrSpec)],
    "dg_incr": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(IncrSpec), _vp, _vp, _vp, _vp, _vp],
    "dg_incr_host": [C.POINTER(IncrSpec), _vp, _i, _i, _i, _vp, _vp, _vp],
    "dg_gridhist_ws_bytes": [C.POINTER(EofFields), _i, C.POINTER(HistSpec)],
    "dg_gridhist": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(HistSpec), _vp, _vp, _vp],
    "dg_gridhist_scan": [_vp, _i, _i, _i, _i, C.POINTER(C.c_double), _i, _vp, _vp, _vp],
    "dg_gridhist_host": [C.POINTER(HistSpec), _vp, _vp, _i, _i, _i, _vp],
    "dg_gridhist_scan_host": [_vp, _i, _i, _i, _i, C.POINTER(C.c_double), _i, _vp, _vp],
    "dg_qmap_fit": [_vp, _i, _i, _i, C.POINTER(_f), C.POINTER(C.c_double), _vp, _vp],
    "dg_qmap_apply": [C.POINTER(EofFields), C.POINTER(HistSpec), _vp, _vp, _vp],
    "dg_qmap_fit_host": [_vp, _i, _i, _i, C.POINTER(_f), C.POINTER(C.c_double), _vp],
    "dg_qmap_apply_host": [C.POINTER(HistSpec), _vp, _i, _i, _i, _vp, _vp],
    "dg_temporal_ws_bytes": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(TemporalSpec)],
    "dg_temporal": [C.POINTER(EofFields), C.POINTER(EofFields), C.POINTER(TemporalSpec), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                    _vp],
    "dg_temporal_host": [C.POINTER(TemporalSpec), _vp, _i, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dg_objects_ws_bytes": [C.POINTER(EofFields), _i, _i, C.POINTER(ObjectsSpec)],
    "dg_objects": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(ObjectsSpec), _vp, _vp, _i64, _vp, _vp, _vp],
    "dg_objects_host": [C.POINTER(ObjectsSpec), _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _vp],
    "dg_distmap_ws_bytes": [C.POINTER(EofFields), _i, _i, C.POINTER(DistmapSpec)],
    "dg_distmap": [C.POINTER(EofFields), C.POINTER(EofFields), _i, _i, C.POINTER(DistmapSpec), _vp, _vp, _vp, _vp, _vp],
    "dg_distmap_host": [C.POINTER(DistmapSpec), _vp, _vp, _i, _i, _i, _vp, _vp, _vp],
    "dg_distmap_host_scalars": [C.c_int32, _i, _vp, _vp, _vp],
}
_RESTYPES = {"dg_rapsd_ws_bytes": C.c_size_t, "dg_cross_rapsd_ws_bytes": C.c_size_t,
             "dg_helmholtz_ws_bytes": C.c_size_t, "dg_helmholtz_cross_ws_bytes": C.c_size_t, "dg_hist_ws_bytes": C.c_size_t, "dg_gridstats_ws_bytes": C.c_size_t,
             "dg_fss_ws_bytes": C.c_size_t, "dg_fss_bound": C.c_int64, "dg_hist2d_ws_bytes": C.c_size_t,
             "dg_incr_ws_bytes": C.c_size_t, "dg_gridhist_ws_bytes": C.c_size_t,
             "dg_temporal_ws_bytes": C.c_size_t, "dg_objects_ws_bytes": C.c_size_t,
             "dg_distmap_ws_bytes": C.c_size_t, "dg_iscale_ws_bytes": C.c_size_t, "dg_iscale_bound": C.c_int64,
             "dg_deform_ws_bytes": C.c_size_t, "dg_deform_bound": C.c_int64}      # every other entry point returns a dg_status
EXPORTS = ["dg_version"] + list(_PROTOS)

_lib = None


def _object_of(handle, symbol="hipGetDeviceCount"):
    """Path of the mapped shared object that ``symbol`` resolves to when looked up through ``handle`` (dlsym searches the object
    and its dependencies, so for a library linked against libamdhip64 this names the HIP runtime its kernels register with)."""
    try:
        addr = C.cast(getattr(handle, symbol), C.c_void_p).value
    except AttributeError:
        return None
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) < 6:
                continue
            lo, hi = (int(x, 16) for x in parts[0].split("-"))
            if lo <= addr < hi:
                return os.path.realpath(parts[5].strip())
    return None


def hip_runtime_binding(l=None):
    """(runtime libdowngan_hip.so is bound to, runtime torch's HIP libraries are bound to); either may be None when it cannot be
    determined (a torch build without HIP libraries)."""
    import torch
    mine = _object_of(l if l is not None else C.CDLL(LIB_PATH))
    c10 = os.path.join(os.path.dirname(torch.__file__), "lib", "libc10_hip.so")
    theirs = _object_of(C.CDLL(c10)) if os.path.exists(c10) else None
    return mine, theirs


def lib():
    """Load (once) and return the shared library; raise loudly when it has not been built, or when it is bound to another HIP
    runtime than torch's."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C downgan_amd/csrc`. downgan_amd has no CPU or eager fallback.")
        # torch first: the library's kernels must register with the HIP runtime torch brings along (its own libamdhip64), the one
        # whose streams and device pointers the C ABI is handed.  Loaded before torch, the library binds /opt/rocm's copy and every
        # launch on a torch stream fails (seen as DG_ERR_LAUNCH from the first kernel when build() and smoke() share a process).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        # ... and verified: a host process that mapped libdowngan_hip.so (or another libamdhip64 with the same soname) BEFORE torch
        # has bound the library to that runtime for good -- say so here instead of failing every launch with DG_ERR_LAUNCH later
        mine, theirs = hip_runtime_binding(l)
        if mine is not None and theirs is not None and mine != theirs:
            raise RuntimeError(
                f"libdowngan_hip.so is bound to the HIP runtime {mine}, torch to {theirs}: two HIP runtimes in one process. The "
                "library's kernels are registered with the first, while the streams and device pointers it is handed belong to the "
                "second, so every launch would fail (DG_ERR_LAUNCH). Import torch (or downgan_amd, which does) before anything that "
                "loads libdowngan_hip.so or /opt/rocm's libamdhip64 into this process.")
        l.dg_version.restype = C.c_char_p
        l.dg_version.argtypes = []
        for name, args in _PROTOS.items():
            fn = getattr(l, name)
            fn.restype = _RESTYPES.get(name, C.c_int)
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {STATUS.get(rc, rc)}")
