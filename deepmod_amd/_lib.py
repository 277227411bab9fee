"""ctypes binding of libdeepmod_hip.so (include/deepmod_hip.h).  No fallbacks: if the HIP
library is missing or no gfx950 device is usable, every entry point raises."""
from __future__ import annotations

import ctypes
import os
import sys
from typing import Optional

# Multi-process GPU work on this stack (RCCL communicators between the ranks of a node) needs the ROCr runtime in its dmabuf IPC mode: the
# host driver does not support the legacy IPC handles, and with them hipIpcGetMemHandle - hence ncclCommInitRank's buffer exchange -
# fails with "invalid argument".  The runtime reads the variable when it initialises (the first HIP call of the process), so it is set
# here, before the library is loaded, unless the caller has decided otherwise.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libdeepmod_hip.so")

DM_OPT_PROFILE = 1
DM_OPT_PRECISION = 2
DM_OPT_ASYNC = 3
DM_OPT_RESERVED_CUS = 4
DM_OPT_F16X3_SHAPE = 5   # 16 (the product: 16x16x32 MFMAs) | 32 (experiment builds only: the 32x32x16 kernels of rounds 2-3)
DM_PREC_F32 = 0
DM_PREC_F16X3 = 1
DM_PREC_F16I8 = 3      # opt-in, reduced precision: int8 cross terms (2 issued matrix units per product instead of 3; worst window of 1e6 1.1e-4 instead of 9e-6 at weight scale 4)
DM_PREC_F16X3_ROLES = 2   # round-4 experiment (matrix / cell wave pairs, bit-identical to F16X3): only in a library built with -DDM_WITH_F16X3_ROLES (DM_INFO_HAS_F16X3_ROLES)
DM_INFO_PRECISION, DM_INFO_F16_REPRESENTABLE, DM_INFO_F16_LENGTH_SHIFT, DM_INFO_DEVICE, DM_INFO_HAS_F16X3_ROLES = 1, 2, 3, 4, 5
DM_INFO_HAS_F16S = 6         # 1: experiment build with the 32x32x16 kernels of rounds 2-3 (DM_WITH_F16S=1)
DM_INFO_GRID_CAP = 7         # most workgroups a classifier launch may use: CUs - DM_OPT_RESERVED_CUS
DM_INFO_LAST_GRID = 8        # workgroups of the model's last classifier launch (0 before the first)
DM_OK, DM_EINVAL, DM_EDEVICE, DM_ENOMEM, DM_ESTATE, DM_ERCCL, DM_ERANGE = 0, -1, -2, -3, -4, -5, -6
(DM_MAP_STATUS, DM_MAP_N_ROWS, DM_MAP_LEFTCLIP, DM_MAP_RIGHTCLIP, DM_MAP_EV_LO, DM_MAP_EV_HI, DM_MAP_FIRST_MATCH_POS,
 DM_MAP_LAST_MATCH_POS, DM_MAP_NUM_INSERT, DM_MAP_NUM_DELETE, DM_MAP_NUM_MISMATCH, DM_MAP_STRAND, DM_MAP_POS_AFTER_CLIP,
 DM_MAP_EVENTS_AFTER_CLIP) = range(14)
DM_MAP_INFO_LEN = 16
DM_MAP_OK, DM_MAP_NO_MATCH, DM_MAP_NEED_ROWS = 0, 1, 2
DM_MOVE_OK, DM_MOVE_COUNT, DM_MOVE_OUTSIDE = 0, 1, 2
(DM_XY_OK, DM_XY_LESS_EVENT, DM_XY_NO_SITE, DM_XY_FILTERED, DM_XY_NO_MATCH, DM_XY_INDEX_ERROR, DM_XY_NEED_ROWS) = range(7)
DM_XY_INFO_LEN = 8
(DM_XY_STATUS, DM_XY_N_ROWS, DM_XY_STRAND, DM_XY_START_CLIP, DM_XY_END_CLIP, DM_XY_POS_AFTER_CLIP, DM_XY_EVENTS_AFTER_CLIP) = range(7)
DM_WEIGHT_FLOATS = 408402

_c = ctypes
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64

# (name, restype, argtypes) — mirrors include/deepmod_hip.h one to one
SIGNATURES = [
    ("dm_last_error", _c.c_char_p, []),
    ("dm_version", _c.c_char_p, []),
    ("dm_build_flags", _c.c_char_p, []),
    ("dm_device_count", _c.c_int, []),
    ("dm_device_pci_bus_id", _c.c_int, [_c.c_int, _c.c_char_p, _c.c_int]),
    ("dm_model_create", _vp, [_c.c_int, _vp, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    ("dm_model_destroy", None, [_vp]),
    ("dm_model_set_option", _c.c_int, [_vp, _c.c_int, _i64]),
    ("dm_model_get_info", _c.c_int, [_vp, _c.c_int, _c.POINTER(_i64)]),
    ("dm_model_calibrate_i8", _c.c_int, [_vp, _i64, _c.c_double, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int)]),
    ("dm_predict_windows", _c.c_int, [_vp, _vp, _i64, _vp, _vp]),
    ("dm_predict_read", _c.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    ("dm_predict_read_at", _c.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    ("dm_model_sync", _c.c_int, [_vp]),
    ("dm_profile_reset", _c.c_int, [_vp]),
    ("dm_profile_get", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_device_alloc", _vp, [_c.c_int, _c.c_size_t]),
    ("dm_device_free", _c.c_int, [_c.c_int, _vp]),
    ("dm_memcpy_h2d", _c.c_int, [_c.c_int, _vp, _vp, _c.c_size_t]),
    ("dm_memcpy_d2h", _c.c_int, [_c.c_int, _vp, _vp, _c.c_size_t]),
    ("dm_model_h2d_async", _c.c_int, [_vp, _vp, _vp, _c.c_size_t]),
    ("dm_model_h2d_ahead", _c.c_int, [_vp, _vp, _vp, _c.c_size_t]),
    ("dm_host_alloc", _vp, [_c.c_int, _c.c_size_t]),
    ("dm_host_free", _c.c_int, [_c.c_int, _vp]),
    ("dm_model_mark", _c.c_int, [_vp, _c.c_int]),
    ("dm_model_wait_mark", _c.c_int, [_vp, _c.c_int]),
    ("dm_summary_create", _vp, [_c.c_int, _i64]),
    ("dm_summary_destroy", None, [_vp]),
    ("dm_summary_length", _i64, [_vp]),
    ("dm_summary_add", _c.c_int, [_vp, _vp, _vp, _i64]),
    ("dm_summary_add_classified", _c.c_int, [_vp, _vp, _vp, _vp, _i64]),
    ("dm_summary_sync", _c.c_int, [_vp]),
    ("dm_summary_grow", _c.c_int, [_vp, _i64]),
    ("dm_rccl_unique_id", _c.c_int, [_vp]),
    ("dm_rccl_info", _c.c_int, [_c.c_char_p, _c.c_int, _c.POINTER(_c.c_int)]),
    ("dm_comm_create", _vp, [_c.c_int, _vp, _c.c_int, _c.c_int]),
    ("dm_comm_destroy", None, [_vp]),
    ("dm_comm_rank", _c.c_int, [_vp]),
    ("dm_comm_size", _c.c_int, [_vp]),
    ("dm_comm_barrier", _c.c_int, [_vp]),
    ("dm_comm_max_f64", _c.c_int, [_vp, _c.POINTER(_c.c_double)]),
    ("dm_comm_stats", _c.c_int, [_vp, _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_summary_reduce", _c.c_int, [_vp, _vp, _c.c_int]),
    ("dm_summary_reduce_scatter", _c.c_int, [_vp, _vp, _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_summary_fetch_slice", _c.c_int, [_vp, _vp, _vp, _vp]),
    ("dm_summary_fetch", _c.c_int, [_vp, _vp, _vp, _vp]),
    ("dm_summary_device_ptr", _vp, [_vp]),
    ("dm_summary_follow", _c.c_int, [_vp, _vp]),
    ("dm_bed_format", _i64, [_c.c_char_p, _c.c_char, _c.c_char, _vp, _vp, _vp, _i64, _vp, _i64]),
    ("dm_bed_format_at", _i64, [_c.c_char_p, _c.c_char, _c.c_char, _i64, _vp, _vp, _vp, _i64, _vp, _i64]),
    ("dm_cluster_create", _vp, [_c.c_int, _vp, _c.c_size_t]),
    ("dm_cluster_destroy", None, [_vp]),
    ("dm_cluster_predict", _c.c_int, [_vp, _vp, _i64, _vp]),
    ("dm_cluster_sites", _i64, [_vp, _vp, _vp, _c.c_int, _vp, _i64, _i64, _i64, _i64, _vp, _c.POINTER(_i64)]),
    ("dm_cluster_sites_fetch", _c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_cluster_bed_format", _i64, [_c.c_char_p, _c.c_char, _c.c_char, _vp, _vp, _vp, _vp, _i64, _vp, _i64]),
    ("dm_signal_create", _vp, [_c.c_int]),
    ("dm_signal_destroy", None, [_vp]),
    ("dm_map_read", _c.c_int, [_c.c_int, _i64, _c.c_char_p, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    ("dm_signal_event_stats", _c.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _c.POINTER(_i64), _vp]),
    ("dm_signal_event_stats_batch", _c.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_signal_plan_batch", _c.c_int, [_i64, _vp, _vp, _vp, _vp, _vp]),
    ("dm_signal_event_stats_device", _c.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_signal_move_stats_device", _c.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_signal_move_chunk", _i64, []),
    ("dm_move_events", _i64, [_i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_events_merge", _i64, [_i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_rows_create", _vp, [_c.c_char]),
    ("dm_rows_destroy", None, [_vp]),
    ("dm_rows_add_packed", _c.c_int, [_vp, _i64, _i64, _i64, _i64, _c.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_rows_add_raw", _c.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int32, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _c.c_int32, _vp, _vp, _vp]),
    ("dm_rows_add_mapped", _c.c_int, [_vp, _i64, _i64, _i64, _c.c_int32] + [_vp] * 16),
    ("dm_rows_info", _i64, [_vp, _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i64), _vp, _vp, _i64, _c.POINTER(_i64)]),
    ("dm_rows_emit", _i64, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _c.POINTER(_c.c_int32)]),
    ("dm_rows_device_info", _c.c_int, [_vp, _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_rows_emit_device", _i64, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _c.POINTER(_c.c_int32)]),
    ("dm_rows_emit_resident", _i64, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _c.POINTER(_c.c_int32)]),
    ("dm_rows_assemble", _c.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64]),
    ("dm_trainer_create", _vp, [_c.c_int, _vp, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _i64]),
    ("dm_trainer_destroy", None, [_vp]),
    ("dm_trainer_grad", _c.c_int, [_vp, _vp, _vp, _i64, _c.c_int, _c.POINTER(_c.c_float), _vp, _vp]),
    ("dm_trainer_adam", _c.c_int, [_vp, _vp]),
    ("dm_trainer_step", _c.c_int, [_vp, _vp, _vp, _i64, _c.c_int, _c.POINTER(_c.c_float)]),
    ("dm_trainer_get_state", _c.c_int, [_vp, _vp, _vp, _vp, _c.POINTER(_i64)]),
    ("dm_trainer_set_state", _c.c_int, [_vp, _vp, _vp, _vp, _i64]),
    ("dm_trainer_profile", _c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_i64)]),
    ("dm_xy_sites_create", _vp, [_c.c_int32, _c.c_int, _c.c_int]),
    ("dm_xy_sites_destroy", None, [_vp]),
    ("dm_xy_sites_set", _c.c_int, [_vp, _c.c_int32, _c.c_int, _c.c_int, _vp, _i64]),
    ("dm_xy_labels", _c.c_int, [_vp, _c.c_int32, _c.c_int, _c.c_char_p, _c.c_int, _c.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64,
                                _i64, _vp, _vp]),
    ("dm_xy_read", _c.c_int, [_vp, _c.c_int32, _c.c_int, _i64, _c.c_char_p, _c.c_char_p, _i64, _c.c_char_p, _i64, _i64, _c.c_char_p, _c.c_int, _c.c_int, _vp, _vp, _vp,
                              _i64, _i64, _i64, _vp, _vp]),
    ("dm_xy_format_host", _i64, [_vp, _i64, _vp, _i64]),
    ("dm_xy_rows_host", _i64, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64]),
    ("dm_xy_create", _vp, [_c.c_int]),
    ("dm_xy_destroy", None, [_vp]),
    ("dm_xy_rows", _i64, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _c.POINTER(_c.c_int32)]),
    ("dm_xy_rows_fetch", _c.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("dm_xy_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_xy_scan", _c.c_int, [_vp, _vp, _i64]),
    ("dm_xyload_create", _vp, [_c.c_int]),
    ("dm_xyload_destroy", None, [_vp]),
    ("dm_xyload_parse", _c.c_int, [_vp, _vp, _i64, _c.POINTER(_i64), _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_xyload_parse_host", _i64, [_vp, _i64, _vp, _i64, _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_xyload_set_table", _c.c_int, [_vp, _vp, _i64]),
    ("dm_xyload_select", _i64, [_vp, _c.c_int, _i64, _i64, _c.POINTER(_i64)]),
    ("dm_xyload_set_selection", _c.c_int, [_vp, _vp, _vp, _i64]),
    ("dm_xyload_device", _c.c_int, [_vp, _c.POINTER(_vp), _c.POINTER(_vp), _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_xyload_fetch", _c.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("dm_xyload_classify", _c.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("dm_xyload_select_host", _i64, [_vp, _i64, _c.c_int, _i64, _i64, _vp, _vp, _i64, _c.POINTER(_i64)]),
    ("dm_xyload_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_xyload_tile_bytes", _c.c_int, []),
    ("dm_xyload_scan_block", _c.c_int, []),
    ("dm_xyset_create", _vp, [_c.c_int, _i64]),
    ("dm_xyset_destroy", None, [_vp]),
    ("dm_xyset_append", _c.c_int, [_vp, _vp]),
    ("dm_xyset_segments", _i64, [_vp, _vp, _vp, _i64]),
    ("dm_xyset_classify", _c.c_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    ("dm_xyset_bytes", _i64, [_vp]),
    ("dm_xyset_gather", _c.c_int, [_vp, _vp, _i64, _vp]),
    ("dm_trainer_step_set", _c.c_int, [_vp, _vp, _vp, _vp, _i64, _c.c_int, _c.POINTER(_c.c_float)]),
    ("dm_trainer_grad_set", _c.c_int, [_vp, _vp, _vp, _vp, _i64, _c.c_int, _c.POINTER(_c.c_float), _vp, _vp]),
    ("dm_cluster_trainer_create", _vp, [_c.c_int, _vp, _c.c_size_t, _i64]),
    ("dm_cluster_trainer_destroy", None, [_vp]),
    ("dm_cluster_trainer_set_data", _c.c_int, [_vp, _vp, _vp, _i64]),
    ("dm_cluster_trainer_grad", _c.c_int, [_vp, _vp, _vp, _i64, _c.c_float, _vp, _c.c_uint64, _i64, _c.POINTER(_c.c_float), _vp, _vp]),
    ("dm_cluster_trainer_adam", _c.c_int, [_vp, _vp]),
    ("dm_cluster_trainer_step", _c.c_int, [_vp, _vp, _i64, _c.c_float, _c.c_uint64]),
    ("dm_cluster_trainer_losses", _c.c_int, [_vp, _i64, _i64, _vp]),
    ("dm_cluster_trainer_mask", _c.c_int, [_vp, _c.c_uint64, _i64, _i64, _c.c_float, _vp]),
    ("dm_cluster_trainer_get_state", _c.c_int, [_vp, _vp, _vp, _vp, _c.POINTER(_i64)]),
    ("dm_cluster_trainer_set_state", _c.c_int, [_vp, _vp, _vp, _vp, _i64]),
    ("dm_siteperf_create", _vp, [_c.c_int, _c.c_int, _vp]),
    ("dm_siteperf_destroy", None, [_vp]),
    ("dm_siteperf_set_contig", _c.c_int, [_vp, _vp, _i64, _c.c_char_p, _c.c_int, _c.c_int, _i64, _i64]),
    ("dm_siteperf_fetch_codes", _c.c_int, [_vp, _vp]),
    ("dm_siteperf_add_text", _c.c_int, [_vp, _vp, _i64, _c.c_int, _c.c_char_p, _c.POINTER(_i64), _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_siteperf_add_records", _c.c_int, [_vp, _c.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_siteperf_fetch_records", _c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_siteperf_finish_contig", _c.c_int, [_vp]),
    ("dm_siteperf_fetch", _c.c_int, [_vp, _vp, _vp, _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_siteperf_parse_host", _i64, [_vp, _i64, _c.c_char_p, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_siteperf_tile_bytes", _c.c_int, []),
    ("dm_siteperf_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_bedmerge_create", _vp, [_c.c_int]),
    ("dm_bedmerge_destroy", None, [_vp]),
    ("dm_bedmerge_open", _c.c_int, [_vp, _vp, _vp, _c.c_char_p, _c.c_int]),
    ("dm_bedmerge_add_text", _c.c_int, [_vp, _vp, _i64, _c.POINTER(_i64), _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_bedmerge_add_records", _c.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    ("dm_bedmerge_fetch_records", _c.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("dm_bedmerge_format_begin", _c.c_int, [_vp, _c.c_char, _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_bedmerge_format_next", _c.c_int, [_vp, _vp, _i64, _c.POINTER(_i64)]),
    ("dm_bedmerge_parse_host", _i64, [_vp, _i64, _c.c_char_p, _i64, _vp, _vp, _vp, _vp, _i64, _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_bedmerge_format_host", _i64, [_c.c_char_p, _c.c_char, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _c.POINTER(_i64)]),
    ("dm_bedmerge_tile_positions", _c.c_int, []),
    ("dm_bedmerge_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_bsperf_create", _vp, [_c.c_int, _c.c_int, _vp, _vp, _c.c_int, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    ("dm_bsperf_destroy", None, [_vp]),
    ("dm_bsperf_add_truth_text", _c.c_int, [_vp, _c.c_int, _vp, _i64, _c.c_int, _vp, _c.POINTER(_i64), _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_bsperf_add_truth_records", _c.c_int, [_vp, _c.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_bsperf_fetch_records", _c.c_int, [_vp, _vp, _vp]),
    ("dm_bsperf_open", _c.c_int, [_vp, _c.c_int, _vp, _vp]),
    ("dm_bsperf_close_contig", _c.c_int, [_vp]),
    ("dm_bsperf_fill", _c.c_int, [_vp, _c.c_int, _i64, _vp, _vp, _c.POINTER(_i64), _c.POINTER(_c.c_int32)]),
    ("dm_bsperf_count", _c.c_int, [_vp]),
    ("dm_bsperf_add_scores", _c.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("dm_bsperf_fetch", _c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_bsperf_parse_host", _i64, [_vp, _i64, _c.c_int, _vp, _vp, _c.c_int, _vp, _vp, _i64, _vp, _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_bsperf_tile_bytes", _c.c_int, []),
    ("dm_bsperf_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_bslabels_create", _vp, [_c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    ("dm_bslabels_destroy", None, [_vp]),
    ("dm_bslabels_add_truth_text", _c.c_int, [_vp, _c.c_int, _vp, _i64, _c.c_int, _vp, _c.POINTER(_i64), _c.POINTER(_c.c_int32), _c.POINTER(_i64)]),
    ("dm_bslabels_add_truth_records", _c.c_int, [_vp, _c.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_bslabels_fetch_records", _c.c_int, [_vp, _vp, _vp]),
    ("dm_bslabels_open", _c.c_int, [_vp, _c.c_int, _vp, _i64, _c.c_char_p, _c.c_int, _c.c_int]),
    ("dm_bslabels_fill", _c.c_int, [_vp, _c.c_int, _i64, _vp, _vp, _c.POINTER(_i64), _c.POINTER(_c.c_int32)]),
    ("dm_bslabels_classify", _c.c_int, [_vp, _vp]),
    ("dm_bslabels_fetch_classes", _c.c_int, [_vp, _vp]),
    ("dm_bslabels_format_begin", _c.c_int, [_vp, _c.c_int, _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i64)]),
    ("dm_bslabels_format_next", _c.c_int, [_vp, _vp, _i64, _c.POINTER(_i64)]),
    ("dm_bslabels_close_contig", _c.c_int, [_vp]),
    ("dm_bslabels_format_host", _i64, [_c.c_char_p, _c.c_int, _vp, _vp, _i64, _i64, _vp, _i64]),
    ("dm_bslabels_tile_positions", _c.c_int, []),
    ("dm_bslabels_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_motifs_create", _vp, [_c.c_int, _c.c_int, _c.c_int, _c.c_char, _c.c_int, _c.c_int, _c.c_int]),
    ("dm_motifs_destroy", None, [_vp]),
    ("dm_motifs_count", _c.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_motifs_fetch", _c.c_int, [_vp, _vp]),
    ("dm_motifs_reset", _c.c_int, [_vp]),
    ("dm_motifs_tile_positions", _c.c_int, []),
    ("dm_motifs_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_motifs_count_host", _c.c_int, [_c.c_int, _c.c_int, _c.c_char, _c.c_int, _c.c_int, _c.c_int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_diffmod_create", _vp, [_c.c_int, _c.c_int, _c.c_double]),
    ("dm_diffmod_destroy", None, [_vp]),
    ("dm_diffmod_run", _c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(_i64)]),
    ("dm_diffmod_fetch_records", _c.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dm_diffmod_fetch_hist", _c.c_int, [_vp, _vp]),
    ("dm_diffmod_reset", _c.c_int, [_vp]),
    ("dm_diffmod_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_diffmod_max_total", _c.c_int, []),
    ("dm_diffmod_tile_positions", _c.c_int, []),
    ("dm_diffmod_small_support", _c.c_int, []),
    ("dm_diffmod_test_host", _c.c_int, [_c.c_int, _c.c_double, _i64] + [_vp] * 10 + [_i64] + [_vp] * 7 + [_c.POINTER(_i64)]),
    ("dm_diffrep_create", _vp, [_c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int]),
    ("dm_diffrep_destroy", None, [_vp]),
    ("dm_diffrep_run", _c.c_int, [_vp, _c.c_int, _c.c_int, _vp, _vp, _vp, _c.POINTER(_i64)]),
    ("dm_diffrep_fetch_records", _c.c_int, [_vp, _i64, _i64] + [_vp] * 10),
    ("dm_diffrep_fetch_hist", _c.c_int, [_vp, _vp]),
    ("dm_diffrep_reset", _c.c_int, [_vp]),
    ("dm_diffrep_times", _c.c_int, [_vp, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("dm_diffrep_max_replicates", _c.c_int, []),
    ("dm_diffrep_test_host", _c.c_int, [_c.c_int, _c.c_double] + [_c.c_int] * 4 + [_i64] + [_vp] * 6 + [_i64] + [_vp] * 10 + [_c.POINTER(_i64)]),
]


class DeepModHipError(RuntimeError):
    code = None


class DeepModRangeError(DeepModHipError):
    """DM_ERANGE: the split-f16 kernel met an input it cannot represent; repeat the call with precision 'f32'."""
    code = DM_ERANGE


_LIB: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load the in-tree HIP library (built by __graft_entry__.build()).  Raises if absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise DeepModHipError(
                "%s not found - build it first (python -c 'import __graft_entry__ as g; g.build()'); "
                "there is no CPU fallback" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, restype, argtypes in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _LIB = lib
    return _LIB


def check(rc: int) -> None:
    if rc != 0:
        msg = "deepmod_hip error %d: %s" % (rc, load().dm_last_error().decode("utf-8", "replace"))
        if rc == DM_ERANGE:
            raise DeepModRangeError(msg)
        err = DeepModHipError(msg)
        err.code = rc
        raise err


def pci_bus_id(device: int) -> str:
    buf = ctypes.create_string_buffer(64)
    check(load().dm_device_pci_bus_id(device, buf, 64))
    return buf.value.decode()


def last_error() -> str:
    return load().dm_last_error().decode("utf-8", "replace")


class Handle:
    """A handle of the C ABI whose entry points are PREFIX_create / PREFIX_destroy / PREFIX_times (N_TIMES doubles): created or DeepModHipError with
    the library's message; close() may be called again and is what __del__ does."""
    PREFIX = None
    N_TIMES = 0

    def _create(self, *args):
        self._ct, self._libmod, self._lib = ctypes, sys.modules[__name__], load()
        self._h = getattr(self._lib, self.PREFIX + "_create")(*args)
        if not self._h:
            raise DeepModHipError(self.PREFIX + "_create: " + last_error())

    def _fn(self, name: str):
        return getattr(self._lib, "%s_%s" % (self.PREFIX, name))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def times(self):
        """ms of the handle's kernels so far, one figure per phase."""
        v = [ctypes.c_double(0.0) for _ in range(self.N_TIMES)]
        check(self._fn("times")(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)
