"""cat_amd/ctc_crf/_C.py -- ctypes binding of libctc_crf_hip.so, mirroring the reference's pybind module
``ctc_crf._C`` (src/ctc_crf/binding.cpp:120-126: gpu_den, gpu_ctc, init_env, release_env).

There is NO CPU fallback and no PyTorch fallback: if the HIP library is missing the import fails,
and every call goes through the C ABI of include/ctc_crf_hip.h.
"""
import ctypes
import os
import sys
import threading
import warnings
from typing import Dict, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRF_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libctc_crf_hip.so")  # CRF_LIB: A/B builds

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the gfx950 HIP library has not been built. "
        "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `python -m cat_amd.build`) first; "
        "there is no CPU fallback for the CTC-CRF loss.")

_lib = ctypes.CDLL(LIB_PATH)

_i64, _i32, _f32, _vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
_lib.crf_graph_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_vp)]
_lib.crf_graph_create.restype = ctypes.c_int
_lib.crf_graph_create_from_arcs.argtypes = [_i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(_vp)]
_lib.crf_graph_create_from_arcs.restype = ctypes.c_int
_lib.crf_graph_destroy.argtypes = [_vp]
_lib.crf_graph_destroy.restype = None
_lib.crf_graph_dims.argtypes = [_vp] + [ctypes.POINTER(_i64)] * 4
_lib.crf_graph_dims.restype = ctypes.c_int
_lib.crf_graph_stats.argtypes = [_vp, ctypes.POINTER(_i64), ctypes.c_int]
_lib.crf_graph_stats.restype = ctypes.c_int
_lib.crf_workspace_bytes.argtypes = [_vp, _i64, _i64, _i64, _i64]
_lib.crf_workspace_bytes.restype = _i64
_lib.crf_den_kernels.argtypes = [_vp, _i64, _i64, _i64]
_lib.crf_den_kernels.restype = ctypes.c_int
_lib.crf_loss_fwd_bwd.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _f32,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_loss_fwd_bwd.restype = ctypes.c_int
_lib.crf_loss_fwd_bwd_logits.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _f32,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_loss_fwd_bwd_logits.restype = ctypes.c_int
_lib.crf_ctc_fwd_bwd.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32,
                                 _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_fwd_bwd.restype = ctypes.c_int
_lib.crf_ctc_fwd_bwd_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32,
                                        _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_fwd_bwd_logits.restype = ctypes.c_int
_lib.crf_ctc_align_logits_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
_lib.crf_ctc_align_logits_workspace_bytes.restype = _i64
_lib.crf_ctc_align_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp,
                                      _vp, _i64, _vp]
_lib.crf_ctc_align_logits.restype = ctypes.c_int
_lib.crf_ctc_align_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
_lib.crf_ctc_align_workspace_bytes.restype = _i64
_lib.crf_ctc_align.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_align.restype = ctypes.c_int
_lib.crf_ctc_score.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]
_lib.crf_ctc_score.restype = ctypes.c_int
_lib.crf_ctc_score_logits_workspace_bytes.argtypes = [_i64, _i64, _i64]
_lib.crf_ctc_score_logits_workspace_bytes.restype = _i64
_lib.crf_ctc_score_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                      _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_score_logits.restype = ctypes.c_int
_lib.crf_last_score_kernel.restype = ctypes.c_char_p
_lib.crf_ctc_score_grad_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_ctc_score_grad_workspace_bytes.restype = _i64
_lib.crf_ctc_score_grad.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp,
                                    _vp, _i64, _vp]
_lib.crf_ctc_score_grad.restype = ctypes.c_int
_lib.crf_ctc_score_grad_logits_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_ctc_score_grad_logits_workspace_bytes.restype = _i64
_lib.crf_ctc_score_grad_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                           _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_score_grad_logits.restype = ctypes.c_int
_lib.crf_last_score_grad_kernel.restype = ctypes.c_char_p
_lib.crf_ctc_score_rows_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64, ctypes.c_int]
_lib.crf_ctc_score_rows_workspace_bytes.restype = _i64
_lib.crf_ctc_score_rows.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp,
                                    _vp, _i64, _vp]
_lib.crf_ctc_score_rows.restype = ctypes.c_int
_lib.crf_ctc_score_grad_rows_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64, ctypes.c_int]
_lib.crf_ctc_score_grad_rows_workspace_bytes.restype = _i64
_lib.crf_ctc_score_grad_rows.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                         _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_score_grad_rows.restype = ctypes.c_int
_lib.crf_debug_score_rows_ws_sections.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.POINTER(_i64), ctypes.c_int]
_lib.crf_debug_score_rows_ws_sections.restype = ctypes.c_int
_lib.crf_debug_score_rows_ws_section_names.argtypes = [ctypes.c_int]
_lib.crf_debug_score_rows_ws_section_names.restype = ctypes.c_char_p
_lib.crf_ctc_sample_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
_lib.crf_ctc_sample_workspace_bytes.restype = _i64
_lib.crf_ctc_sample.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, ctypes.c_uint64, ctypes.c_uint32,
                                ctypes.c_int, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_sample.restype = ctypes.c_int
_lib.crf_last_sample_kernel.restype = ctypes.c_char_p
_lib.crf_ctc_beam_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_ctc_beam_workspace_bytes.restype = _i64
_lib.crf_ctc_beam.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                              _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_beam.restype = ctypes.c_int
_lib.crf_last_beam_kernel.restype = ctypes.c_char_p
_lib.crf_ngram_tables_check.argtypes = [_vp]
_lib.crf_ngram_tables_check.restype = ctypes.c_int
_lib.crf_ctc_beam_lm_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_ctc_beam_lm_workspace_bytes.restype = _i64
_lib.crf_ctc_beam_lm.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                 _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_beam_lm.restype = ctypes.c_int
_lib.crf_ctc_beam_state_record_bytes.argtypes = [_i64, _i64]
_lib.crf_ctc_beam_state_record_bytes.restype = _i64
_lib.crf_ctc_beam_chunk_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_ctc_beam_chunk_workspace_bytes.restype = _i64
_lib.crf_ctc_beam_chunk.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                    _vp, _f32, _f32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctc_beam_chunk.restype = ctypes.c_int
_lib.crf_ctc_edit_distance.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]
_lib.crf_ctc_edit_distance.restype = ctypes.c_int
_lib.crf_last_edit_kernel.restype = ctypes.c_char_p
_lib.crf_ngram_score.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]
_lib.crf_ngram_score.restype = ctypes.c_int
_lib.crf_last_ngram_score_kernel.restype = ctypes.c_char_p
_lib.crf_rnnt_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _i64]
_lib.crf_rnnt_workspace_bytes.restype = _i64
_lib.crf_rnnt_loss.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_loss.restype = ctypes.c_int
_lib.crf_rnnt_loss_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_loss_logits.restype = ctypes.c_int
_lib.crf_rnnt_grad.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_grad.restype = ctypes.c_int
_lib.crf_rnnt_grad_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_grad_logits.restype = ctypes.c_int
_lib.crf_debug_rnnt_ws_sections.argtypes = [_i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.c_int]
_lib.crf_debug_rnnt_ws_sections.restype = ctypes.c_int
_lib.crf_debug_rnnt_ws_section_names.restype = ctypes.c_char_p
_lib.crf_rnnt_simple_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
_lib.crf_rnnt_simple_workspace_bytes.restype = _i64
_lib.crf_rnnt_simple_loss.argtypes = [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_simple_loss.restype = ctypes.c_int
_lib.crf_rnnt_simple_grad.argtypes = [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
_lib.crf_rnnt_simple_grad.restype = ctypes.c_int
_lib.crf_debug_rnnt_simple_ws_sections.argtypes = [_i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.c_int]
_lib.crf_debug_rnnt_simple_ws_sections.restype = ctypes.c_int
_lib.crf_debug_rnnt_simple_ws_section_names.restype = ctypes.c_char_p
_lib.crf_ctct_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
_lib.crf_ctct_workspace_bytes.restype = _i64
_lib.crf_ctct_loss.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctct_loss.restype = ctypes.c_int
_lib.crf_ctct_loss_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctct_loss_logits.restype = ctypes.c_int
_lib.crf_ctct_grad.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctct_grad.restype = ctypes.c_int
_lib.crf_ctct_grad_logits.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
_lib.crf_ctct_grad_logits.restype = ctypes.c_int
_lib.crf_debug_ctct_ws_sections.argtypes = [_i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.c_int]
_lib.crf_debug_ctct_ws_sections.restype = ctypes.c_int
_lib.crf_debug_ctct_ws_section_names.restype = ctypes.c_char_p
_lib.crf_profile_enable.argtypes = [ctypes.c_int]
_lib.crf_profile_enable.restype = None
_lib.crf_profile_read.argtypes = [ctypes.POINTER(_f32), ctypes.c_int]
_lib.crf_profile_read.restype = ctypes.c_int
_lib.crf_timing_read.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
_lib.crf_timing_read.restype = ctypes.c_int
_lib.crf_stage_i32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
_lib.crf_stage_i32.restype = ctypes.c_int
_lib.crf_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int]
_lib.crf_debug_set.restype = ctypes.c_int
_lib.crf_debug_unset.argtypes = [ctypes.c_char_p]
_lib.crf_debug_unset.restype = ctypes.c_int
_lib.crf_debug_list.restype = ctypes.c_char_p
_lib.crf_last_error.restype = ctypes.c_char_p
_lib.crf_last_den_kernel.restype = ctypes.c_char_p
_lib.crf_last_call_streams.restype = ctypes.c_int
_lib.crf_last_side_stream.restype = ctypes.c_char_p
_lib.crf_last_fallback_counts.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
_lib.crf_last_fallback_counts.restype = ctypes.c_int
_lib.crf_version.restype = ctypes.c_char_p
_lib.crf_build_switches.restype = ctypes.c_char_p

EXPORTED_SYMBOLS = (
    "crf_graph_create", "crf_graph_create_from_arcs", "crf_graph_destroy", "crf_graph_dims", "crf_graph_stats",
    "crf_workspace_bytes", "crf_den_kernels", "crf_debug_stream_check", "crf_debug_decode_check", "crf_debug_facbatch_check", "crf_debug_fac_emulate", "crf_debug_res_emulate", "crf_debug_stage_plan", "crf_debug_ws_sections", "crf_debug_ws_section_names", "crf_debug_ws_fields", "crf_debug_ws_field_names", "crf_debug_align_ws_sections", "crf_debug_align_ws_section_names", "crf_loss_fwd_bwd", "crf_loss_fwd_bwd_logits", "crf_ctc_fwd_bwd", "crf_ctc_fwd_bwd_logits", "crf_ctc_align_workspace_bytes", "crf_ctc_align", "crf_ctc_align_logits_workspace_bytes", "crf_ctc_align_logits", "crf_ctc_score", "crf_ctc_score_logits_workspace_bytes", "crf_ctc_score_logits", "crf_last_score_kernel", "crf_ctc_score_grad_workspace_bytes", "crf_ctc_score_grad", "crf_ctc_score_grad_logits_workspace_bytes", "crf_ctc_score_grad_logits", "crf_last_score_grad_kernel", "crf_ctc_score_rows_workspace_bytes", "crf_ctc_score_rows", "crf_ctc_score_grad_rows_workspace_bytes", "crf_ctc_score_grad_rows", "crf_debug_score_rows_ws_sections", "crf_debug_score_rows_ws_section_names", "crf_ctc_sample_workspace_bytes", "crf_ctc_sample", "crf_last_sample_kernel", "crf_ctc_beam_workspace_bytes", "crf_ctc_beam", "crf_last_beam_kernel", "crf_ngram_tables_check", "crf_ctc_beam_lm_workspace_bytes", "crf_ctc_beam_lm", "crf_ctc_beam_state_record_bytes", "crf_ctc_beam_chunk_workspace_bytes", "crf_ctc_beam_chunk", "crf_ctc_edit_distance", "crf_last_edit_kernel", "crf_ngram_score", "crf_last_ngram_score_kernel", "crf_rnnt_workspace_bytes", "crf_rnnt_loss", "crf_rnnt_loss_logits", "crf_rnnt_grad", "crf_rnnt_grad_logits", "crf_debug_rnnt_ws_sections", "crf_debug_rnnt_ws_section_names", "crf_rnnt_simple_workspace_bytes", "crf_rnnt_simple_loss", "crf_rnnt_simple_grad", "crf_debug_rnnt_simple_ws_sections", "crf_debug_rnnt_simple_ws_section_names", "crf_ctct_workspace_bytes", "crf_ctct_loss", "crf_ctct_loss_logits", "crf_ctct_grad", "crf_ctct_grad_logits", "crf_debug_ctct_ws_sections", "crf_debug_ctct_ws_section_names", "crf_profile_enable", "crf_profile_read", "crf_timing_read", "crf_stage_i32",
    "crf_debug_set", "crf_debug_unset", "crf_debug_list", "crf_last_den_kernel", "crf_last_call_streams", "crf_last_side_stream", "crf_last_fallback_counts", "crf_build_switches", "crf_last_error", "crf_version",
)

PROFILE_SLOTS = ("prep", "den_fwd_chain", "den_bwd_chain", "ctc_fwd_chain", "ctc_bwd_chain", "grad",
                 "finalize", "call")


def profile_enable(on: bool) -> None:
    _lib.crf_profile_enable(1 if on else 0)


def profile_read() -> Dict[str, float]:
    """Per-kernel HIP-event durations (ms) of the last loss_fwd_bwd call on this thread."""
    buf = (_f32 * 8)()
    n = _lib.crf_profile_read(buf, 8)
    return {PROFILE_SLOTS[i]: float(buf[i]) for i in range(n)}


def last_den_kernel() -> str:
    """Template instantiation of the denominator recursions' kernel in this thread's last call (include/ctc_crf_hip.h)."""
    return _lib.crf_last_den_kernel().decode()


def last_score_kernel() -> str:
    """Template instantiation of the kernel of this thread's last ctc_score call (include/ctc_crf_hip.h crf_last_score_kernel); on device
    rows, where every hypothesis takes the kernel of its own length class, the highest class launched (the bound's)."""
    return _lib.crf_last_score_kernel().decode()


def last_score_grad_kernel() -> str:
    """Template instantiation of the alpha pass of this thread's last ctc_score_grad call (include/ctc_crf_hip.h crf_last_score_grad_kernel);
    a fused call's carries its element type: "crf_ctc_score_grad_alpha_raw_kernel<4, bf16>"; on device rows the highest class launched,
    "crf_rows_grad_alpha_kernel<8>" / "crf_rows_grad_alpha_raw_kernel<8, bf16>"."""
    return _lib.crf_last_score_grad_kernel().decode()


def last_sample_kernel() -> str:
    """Template instantiation of the row kernel of this thread's last ctc_sample call (include/ctc_crf_hip.h crf_last_sample_kernel)."""
    return _lib.crf_last_sample_kernel().decode()


def last_beam_kernel() -> str:
    """Template instantiation of the row kernel of this thread's last ctc_beam_search call (include/ctc_crf_hip.h crf_last_beam_kernel)."""
    return _lib.crf_last_beam_kernel().decode()


def last_edit_kernel() -> str:
    """Template instantiation of the kernel of this thread's last ctc_edit_distance call (include/ctc_crf_hip.h crf_last_edit_kernel)."""
    return _lib.crf_last_edit_kernel().decode()


def last_ngram_score_kernel() -> str:
    """Template instantiation of the kernel of this thread's last ngram_score call (include/ctc_crf_hip.h crf_last_ngram_score_kernel)."""
    return _lib.crf_last_ngram_score_kernel().decode()


def last_call_streams() -> int:
    """1 / 2 / 3: streams this thread's last call put work on (caller's, + side stream, + third stream)."""
    return int(_lib.crf_last_call_streams())


def last_side_stream() -> str:
    """Kind of the side stream of the last call's context and how many candidates were probed (include/ctc_crf_hip.h)."""
    return _lib.crf_last_side_stream().decode()


def last_fallback_counts(stream: int = 0):
    """(denominator, numerator): utterances of this thread's last call that a fallback redid.  Synchronises `stream` -- diagnostics only."""
    buf = (ctypes.c_int32 * 2)()
    _check(_lib.crf_last_fallback_counts(buf, _vp(stream)))
    return int(buf[0]), int(buf[1])


_SERIAL_WARNED = False
_SIDE_STREAM_SEEN = set()      # (device, stream) contexts whose side stream has been looked at: the check costs one set lookup per step afterwards


def _warn_if_serial(key=None) -> None:
    """The library found no stream that runs beside the caller's: every kernel of the loss runs one after the other on the caller's
    stream -- same results, about 1.6 x the step time at the benchmark shape.  The C library says so on stderr (once per context); a
    training script sees it here, once per process, where Python's warning filters and loggers can pick it up."""
    global _SERIAL_WARNED
    if _SERIAL_WARNED or key in _SIDE_STREAM_SEEN:
        return
    if key is not None:
        _SIDE_STREAM_SEEN.add(key)
    desc = _lib.crf_last_side_stream().decode()
    if desc.startswith("none"):
        _SERIAL_WARNED = True
        warnings.warn(f"ctc_crf: no HIP stream of this process runs beside the caller's stream (side stream: {desc}); the CTC-CRF loss runs its "
                      "kernels one after the other -- correct, but about 1.6x slower than the two-stream schedule. Usual cause: every hardware "
                      "queue of the process is shared with the caller's stream (GPU_MAX_HW_QUEUES too small).", RuntimeWarning, stacklevel=3)


def version() -> str:
    return _lib.crf_version().decode()


def build_switches() -> Dict[str, int]:
    """The build-time geometry dials (and TIMING) of the loaded library (include/ctc_crf_hip.h crf_build_switches)."""
    return {k: int(v) for k, v in (kv.split("=") for kv in _lib.crf_build_switches().decode().split())}


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"ctc_crf_hip error {rc}: {_lib.crf_last_error().decode()}")


# Debug / experiment switches of tests and tools (include/ctc_crf_hip.h crf_debug_set): the LIBRARY never reads the
# environment.  For the tools' convenience this binding applies CRF_DEBUG="name=value,name=value" once, at import.
_DEBUG_SET: Dict[str, int] = {}


def debug_set(key: str, value: Optional[int]) -> None:
    """Set (value None: return to the default) one switch of crf_debug_list()."""
    if value is None:
        _check(_lib.crf_debug_unset(key.encode()))
        _DEBUG_SET.pop(key, None)
    else:
        _check(_lib.crf_debug_set(key.encode(), int(value)))
        _DEBUG_SET[key] = int(value)


def debug_list() -> str:
    return _lib.crf_debug_list().decode()


class debug_opts:
    """``with debug_opts(no_factored=1, bat_ul=16): ...`` -- switches set for the block, previous values restored after."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: _DEBUG_SET.get(k) for k in self.kw}
        for k, v in self.kw.items():
            debug_set(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            debug_set(k, v)


# process-global graphs, one per device -- the reference keeps one graph per process in globals
# indexed by DEVICE_HASH[cudaGetDevice()] (den_calculate.cu:263-273, 436-438).  Identified by a GENERATION number, not by
# the handle's value: a later graph can be allocated at the address of one that was destroyed, and a context that compared
# pointers would then take the newcomer for its own (and destroy it).
_GRAPHS: Dict[int, int] = {}
_GRAPH_GEN: Dict[int, int] = {}
_gen_counter = 0


def graph_generation(dev: int) -> Optional[int]:
    """Generation number of the graph currently loaded on `dev` (None: none)."""
    return _GRAPH_GEN.get(dev)


def graph_dims(handle: int):
    S, A, P, ML = _i64(), _i64(), _i64(), _i64()
    _check(_lib.crf_graph_dims(_vp(handle), S, A, P, ML))
    return dict(S=S.value, A=A.value, P=P.value, max_label=ML.value)


def graph_stats(handle: int):
    buf = (_i64 * 27)()
    _check(_lib.crf_graph_stats(_vp(handle), buf, 27))
    k = ("S", "A", "P", "Pr", "Sr", "fwd_ell_arcs", "bwd_ell_arcs", "fwd_bank_conflicts", "bwd_bank_conflicts", "deg",
         "res_K", "res_fwd_slots", "res_bwd_slots", "res_fwd_bank_conflicts", "res_bwd_bank_conflicts", "res_rows",
         "fac", "fac_matched_pairs", "regauged", "fac_tail_rows", "fac_fwd_slots", "fac_bwd_slots", "fac_fused_rows", "fac_G", "fac_geom", "fac_chunks", "facp")
    d = dict(zip(k, [int(x) for x in buf]))
    d["max_in_deg"], d["max_out_deg"] = d["deg"] // 100000, d.pop("deg") % 100000
    d["res_fwd_rows"], d["res_bwd_rows"] = d["res_rows"] // 100000, d.pop("res_rows") % 100000
    d["fac_Gf"], d["fac_Gb"] = d["fac_G"] // 100000, d.pop("fac_G") % 100000
    return d


def den_kernels(handle: int, B: int, T: int, V: int) -> str:
    """Which denominator kernels a call of this shape takes (include/ctc_crf_hip.h crf_den_kernels)."""
    k = _lib.crf_den_kernels(_vp(handle), B, T, V)
    if k < 0:
        _check(1)
    return ("streaming", "resident", "factored", "batch")[k]


def debug_stream_check(handle: int, UL: int, want: int):
    """Host-side construction + self-check of the utterance-minor arc streams (include/ctc_crf_hip.h)."""
    out = (_i64 * 4)()
    _lib.crf_debug_stream_check.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_i64)]
    _lib.crf_debug_stream_check.restype = ctypes.c_int
    _check(_lib.crf_debug_stream_check(_vp(handle), UL, want, out))
    return {"tasks": int(out[0]), "rest_rows": int(out[1]), "steps": int(out[2]), "arc_records": int(out[3])}


def debug_facbatch_check(handle: int):
    """Host-side check of the factored rows of the utterance-minor kernels (include/ctc_crf_hip.h)."""
    out = (_i64 * 4)()
    _lib.crf_debug_facbatch_check.argtypes = [_vp, ctypes.POINTER(_i64)]
    _lib.crf_debug_facbatch_check.restype = ctypes.c_int
    _check(_lib.crf_debug_facbatch_check(_vp(handle), out))
    return {"NU": int(out[0]), "fwd_records": int(out[1]), "bwd_records": int(out[2]), "arcs": int(out[3])}


def debug_fac_emulate(handle: int, T: int = 6, seed: int = 1):
    """CPU emulation of the factored recursion kernels on the layout tables (include/ctc_crf_hip.h): (plain, forward, backward)."""
    out = (ctypes.c_double * 3)()
    _lib.crf_debug_fac_emulate.argtypes = [_vp, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_double)]
    _lib.crf_debug_fac_emulate.restype = ctypes.c_int
    _check(_lib.crf_debug_fac_emulate(_vp(handle), T, seed, out))
    return float(out[0]), float(out[1]), float(out[2])


def debug_stage_plan(T: int, B: int):
    """The stage plan of the staged grad pass (include/ctc_crf_hip.h: crf_debug_stage_plan; no GPU) under the current debug switches."""
    n = 18
    out = (ctypes.c_int32 * (4 + 4 * n))()
    _lib.crf_debug_stage_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    _lib.crf_debug_stage_plan.restype = ctypes.c_int
    _check(_lib.crf_debug_stage_plan(T, B, out, len(out)))
    ns = int(out[0])
    arr = lambda j: [int(out[4 + j * n + k]) for k in range(n)]
    return {"nstage": ns, "piece": int(out[1]), "one_launch": bool(out[2]), "workgroups": int(out[3]),
            "bound": arr(0)[:ns + 1], "poff": arr(1)[:ns + 2], "fpb": arr(2)[:ns + 1], "nf": arr(3)[:ns + 1]}


def debug_res_emulate(handle: int, T: int = 6, seed: int = 1):
    """CPU emulation of the generic register-resident kernels on the layout tables: (plain, forward, backward)."""
    out = (ctypes.c_double * 3)()
    _lib.crf_debug_res_emulate.argtypes = [_vp, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_double)]
    _lib.crf_debug_res_emulate.restype = ctypes.c_int
    _check(_lib.crf_debug_res_emulate(_vp(handle), T, seed, out))
    return float(out[0]), float(out[1]), float(out[2])


def debug_ws_sections(handle: Optional[int], B: int, T: int, V: int, max_label_len: int):
    """[(name, offset, bytes)] of the loss call's workspace in layout order under the current switches (include/ctc_crf_hip.h:
    crf_debug_ws_sections; no GPU; handle None / 0: a numerator-only call)."""
    _lib.crf_debug_ws_sections.argtypes = [_vp, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.c_int]
    _lib.crf_debug_ws_sections.restype = ctypes.c_int
    _lib.crf_debug_ws_section_names.restype = ctypes.c_char_p
    names = _lib.crf_debug_ws_section_names().decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_ws_sections(_vp(handle or 0), B, T, V, max_label_len, out, len(out))
    assert n == len(names), (n, names)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def debug_ws_fields(section: str, n: int):
    """[(name, offset, bytes, element bytes)] of the arrays inside section "pb", "xch" (from the end of its granules) or "bsm" for a batch
    of n (bsm: Bp) utterances (include/ctc_crf_hip.h: crf_debug_ws_fields; no GPU)."""
    _lib.crf_debug_ws_fields.argtypes = [ctypes.c_char_p, _i64, ctypes.POINTER(_i64), ctypes.c_int]
    _lib.crf_debug_ws_fields.restype = ctypes.c_int
    _lib.crf_debug_ws_field_names.argtypes = [ctypes.c_char_p]
    _lib.crf_debug_ws_field_names.restype = ctypes.c_char_p
    names = _lib.crf_debug_ws_field_names(section.encode())
    if names is None:
        _check(1)
    names = names.decode().split(",")
    out = (_i64 * (3 * len(names)))()
    k = _lib.crf_debug_ws_fields(section.encode(), n, out, len(out))
    assert k == len(names), (k, names)
    return [(names[i], int(out[3 * i]), int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(k)]


def debug_align_ws_sections(logits: bool, B: int, T: int, V: int, max_label_len: int):
    """The same for the workspace of crf_ctc_align (logits False: the back-pointer words) / crf_ctc_align_logits (True: + the lse values)."""
    _lib.crf_debug_align_ws_sections.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.c_int]
    _lib.crf_debug_align_ws_sections.restype = ctypes.c_int
    _lib.crf_debug_align_ws_section_names.restype = ctypes.c_char_p
    names = _lib.crf_debug_align_ws_section_names().decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_align_ws_sections(1 if logits else 0, B, T, V, max_label_len, out, len(out))
    if n < 0:
        _check(1)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def debug_score_rows_ws_sections(grad: bool, B: int, H: int, T: int, V: int, len_cap: int, dtype: int = -1):
    """The same for the workspace of crf_ctc_score_rows (grad False) / crf_ctc_score_grad_rows (True); dtype -1: fp32 log-probs, 0 / 1 / 2: raw
    network output in f32 / bf16 / f16 (+ the lse values)."""
    names = _lib.crf_debug_score_rows_ws_section_names(1 if grad else 0).decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_score_rows_ws_sections(1 if grad else 0, B, H, T, V, len_cap, dtype, out, len(out))
    if n < 0:
        _check(1)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def debug_rnnt_ws_sections(N: int, T: int, U1: int, V: int, compact_rows: int = -1):
    """The same for the workspace of crf_rnnt_loss / crf_rnnt_grad (compact_rows < 0: the padded layout)."""
    names = _lib.crf_debug_rnnt_ws_section_names().decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_rnnt_ws_sections(N, T, U1, V, compact_rows, out, len(out))
    if n < 0:
        _check(1)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def debug_rnnt_simple_ws_sections(N: int, T: int, U1: int, V: int):
    """The same for the workspace of crf_rnnt_simple_loss / crf_rnnt_simple_grad."""
    names = _lib.crf_debug_rnnt_simple_ws_section_names().decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_rnnt_simple_ws_sections(N, T, U1, V, out, len(out))
    if n < 0:
        _check(1)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def debug_ctct_ws_sections(N: int, T: int, U1: int, V: int):
    """The same for the workspace of crf_ctct_loss / crf_ctct_grad."""
    names = _lib.crf_debug_ctct_ws_section_names().decode().split(",")
    out = (_i64 * (2 * len(names)))()
    n = _lib.crf_debug_ctct_ws_sections(N, T, U1, V, out, len(out))
    if n < 0:
        _check(1)
    return [(names[k], int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]


def timing_read(n: int = 16384):
    """In-kernel phase stamps of the last call (timing builds only; [] in a product build)."""
    buf = (ctypes.c_uint64 * n)()
    k = _lib.crf_timing_read(buf, n)
    return [int(buf[i]) for i in range(k)]


def compile_graph_host_only(fst_name: str) -> int:
    """Compile the tables on the host only (device = -1): diagnostics and CPU-side tests."""
    out = _vp()
    _check(_lib.crf_graph_create(os.fsencode(fst_name), -1, ctypes.byref(out)))
    return out.value


def init_env(fst_name: str, gpus: torch.Tensor) -> None:
    """binding.cpp:51-56 ``init_env`` -> Init(): load den_lm once per listed GPU."""
    for dev in [int(i) for i in gpus.tolist()]:
        out = _vp()
        _check(_lib.crf_graph_create(os.fsencode(fst_name), dev, ctypes.byref(out)))
        if dev in _GRAPHS:  # the reference leaks on a second Init; we replace
            _lib.crf_graph_destroy(_vp(_GRAPHS.pop(dev)))
        global _gen_counter
        _gen_counter += 1
        _GRAPHS[dev] = out.value
        _GRAPH_GEN[dev] = _gen_counter


def release_env(gpus: torch.Tensor) -> None:
    """binding.cpp:58-63 ``release_env`` -> Release()."""
    for dev in [int(i) for i in gpus.tolist()]:
        h = _GRAPHS.pop(dev, None)
        _GRAPH_GEN.pop(dev, None)
        if h is not None:
            _lib.crf_graph_destroy(_vp(h))


def release_handles(handles: Dict[int, int]) -> None:
    """Release exactly the graphs a CRFContext created ({device: generation}): a device whose graph has been replaced
    since (a second CRFContext on the same device) is left alone -- the replacement already destroyed the old tables."""
    for dev, gen in handles.items():
        if _GRAPH_GEN.get(dev) == gen:
            _GRAPH_GEN.pop(dev)
            _lib.crf_graph_destroy(_vp(_GRAPHS.pop(dev)))


def graph_for(device: torch.device) -> int:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    h = _GRAPHS.get(idx)
    if h is None:
        raise RuntimeError(
            f"no denominator graph loaded on cuda:{idx}: create ctc_crf.CRFContext(den_lm, {idx}) first "
            "(reference: cat/ctc/train.py:137-141)")
    return h


def _ptr(t: Optional[torch.Tensor]):
    return _vp(0) if t is None else _vp(t.data_ptr())


class _PinnedRing:
    """A few pinned int32 staging buffers per device, reused round-robin: a copy from PAGEABLE memory makes the
    host wait for the stream (the next call could not be enqueued while this one runs).  The device copy is
    made by a KERNEL that reads the pinned buffer (crf_stage_i32): a DMA copy in the caller's stream left the
    GPU idle for ~0.15 ms between two calls while the copy engine started (rocprofv3 timeline), and a copy
    stream of its own would be the process's fifth stream -- HIP maps streams onto four hardware queues, two of
    the loss's own side streams then share one and the numerator recursions run one after the other.
    A slot is reused only after the event of its last copy has completed; host threads take slots under a lock."""

    SLOTS = 8

    def __init__(self):
        self.buf = [None] * self.SLOTS
        self.ev = [None] * self.SLOTS
        self.i = 0
        self.lock = threading.Lock()

    def stage(self, src: torch.Tensor, dev: torch.device) -> torch.Tensor:
        with self.lock:
            return self._stage(src, dev)

    def _stage(self, src: torch.Tensor, dev: torch.device) -> torch.Tensor:
        k = self.i
        self.i = (k + 1) % self.SLOTS
        n = src.numel()
        if self.ev[k] is not None:
            self.ev[k].synchronize()
        if self.buf[k] is None or self.buf[k].numel() < n:
            self.buf[k] = torch.empty(max(n, 4096), dtype=torch.int32).pin_memory()
        self.buf[k][:n].copy_(src)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        cur = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _check(_lib.crf_stage_i32(_vp(out.data_ptr()), _vp(self.buf[k].data_ptr()), n, _vp(cur.cuda_stream)))
        ev = torch.cuda.Event()
        ev.record(cur)
        self.ev[k] = ev
        return out


_RINGS = {}


def _h2d_async(src: torch.Tensor, dev: torch.device) -> torch.Tensor:
    if src.is_cuda:
        return src
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ring = _RINGS.get(key)
    if ring is None:
        ring = _RINGS.setdefault(key, _PinnedRing())
    return ring.stage(src, dev)


_FUSED_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

# Debug aid for the parity tests (set_debug_poison): fill the workspace with NaN bit patterns before every call, so
# that a kernel reading a row before its producer has written it cannot pass by finding the previous call's values in the
# block the caching allocator hands back.
_POISON_WS = False


def set_debug_poison(on: bool) -> None:
    global _POISON_WS
    _POISON_WS = bool(on)


def _validate_meta(lx_cpu, ly_cpu, lab_cpu, T: int, V: int, blank: int = 0) -> None:
    """Host-resident metadata is checked before the launch (no device sync: these tensors are on the CPU already).
    The reference does not check: lx > T walks past the buffers, a label >= V indexes the logits out of bounds
    (gpu_ctc_kernels.h:146-152 reads probs[... + label])."""
    if lx_cpu.numel() and (int(lx_cpu.min()) < 0 or int(lx_cpu.max()) > T):
        raise RuntimeError(f"frame lengths must lie in [0, T={T}], got [{int(lx_cpu.min())}, {int(lx_cpu.max())}]")
    if ly_cpu is not None:
        if ly_cpu.numel() and int(ly_cpu.min()) < 0:
            raise RuntimeError("negative label length")
        if int(ly_cpu.sum()) > lab_cpu.numel():
            raise RuntimeError(f"sum(label_lengths)={int(ly_cpu.sum())} exceeds len(labels)={lab_cpu.numel()}")
        n = int(ly_cpu.sum())
        if blank == 0:
            if n and (int(lab_cpu[:n].min()) <= 0 or int(lab_cpu[:n].max()) >= V):
                raise RuntimeError(f"labels must lie in [1, V-1={V - 1}] (0 is the blank), got [{int(lab_cpu[:n].min())}, {int(lab_cpu[:n].max())}]")
        elif n and (int(lab_cpu[:n].min()) < 0 or int(lab_cpu[:n].max()) >= V or bool((lab_cpu[:n] == blank).any())):
            raise RuntimeError(f"labels must lie in [0, V-1={V - 1}] without the blank {blank}, got [{int(lab_cpu[:n].min())}, {int(lab_cpu[:n].max())}]"
                               + (" and the blank itself" if bool((lab_cpu[:n] == blank).any()) else ""))


def _act_shape(t: torch.Tensor, fused: bool, time_major: bool, blank: int):
    """The activations' dtype check (fused: raw network output in f32 / bf16 / f16, else f32 log-probs), their shape with the
    time_major swap and the blank's range.  -> (device, N, T, V)."""
    if fused:
        if t.dtype not in _FUSED_DTYPES:
            raise RuntimeError(f"fused log_softmax: expect float32, bfloat16 or float16 network output, got {t.dtype}")
    else:
        assert t.dtype == torch.float32
    N, T, V = t.shape
    if time_major:
        T, N = N, T
    if not 0 <= blank < V:
        raise RuntimeError(f"blank must lie in [0, V-1={V - 1}], got {blank}")
    return t.device, N, T, V


def _new_ws(nbytes: int, dev: torch.device) -> torch.Tensor:
    """A call's workspace; nbytes < 0: the size function has refused the shape and left its message."""
    if nbytes < 0:
        _check(1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if _POISON_WS:
        ws.fill_(0xFF)   # every float / double / int32 of the workspace reads as NaN / -1
    return ws


def loss_fwd_bwd(logits: torch.Tensor, labels: Optional[torch.Tensor], lx: torch.Tensor,
                 ly: Optional[torch.Tensor], c_den: float, c_ctc: float, graph: Optional[int],
                 want_costs: bool = False, fused: bool = False, time_major: bool = False, blank: int = 0,
                 grad_out: Optional[torch.Tensor] = None):
    """One call of the hot path (include/ctc_crf_hip.h ``crf_loss_fwd_bwd``).

    logits [N,T,V] f32 on the GPU, contiguous; labels/lx/ly int32 on CPU (as CAT passes them,
    cat/ctc/train.py:176-190) or on the GPU.  Returns (loss[1], grad[N,T,V], extras dict).
    Numerator-only calls (c_den == 0; ``crf_ctc_fwd_bwd``, fused: ``crf_ctc_fwd_bwd_logits``) also take time_major=True -- logits and
    the returned gradient are [T,N,V] -- and any blank column in [0, V); grad_out: a contiguous f32 tensor of logits'
    shape that receives the gradient (else one is allocated).
    """
    assert logits.is_cuda and logits.is_contiguous() and logits.dim() == 3
    if (time_major or blank != 0) and c_den != 0.0:
        raise RuntimeError("time_major and a blank other than 0 are for numerator-only calls (WARP_CTC_LOSS / gpu_ctc): "
                           "the den_lm fixes the blank at 0 and the CTC-CRF kernels read [N,T,V] log-probs")
    dev, N, T, V = _act_shape(logits, fused, time_major, blank)   # fused: raw network output (crf_loss_fwd_bwd_logits)
    lx32 = lx.to(torch.int32)
    if c_ctc != 0.0:
        ly32 = ly.to(torch.int32)
        ly_cpu = ly32.cpu()
        max_l = int(ly_cpu.max()) if N > 0 else 0
        off = (torch.cumsum(ly_cpu, 0, dtype=torch.int32) - ly_cpu).to(torch.int32)
        lab32 = labels.to(torch.int32).reshape(-1)
        if not lx32.is_cuda and not lab32.is_cuda:
            _validate_meta(lx32, ly_cpu, lab32, T, V, blank)
        if lab32.numel() == 0:
            lab32 = torch.zeros(1, dtype=torch.int32)
        # one H2D copy for all integer metadata (the reference issues ~5, gpu_ctc.h:143-229), through pinned
        # staging so that it does not serialise the host with the stream
        meta = _h2d_async(torch.cat([lx32.cpu().reshape(-1), ly_cpu.reshape(-1), off.reshape(-1), lab32.cpu()]), dev)
        lx_d, ly_d, off_d, lab_d = meta[:N], meta[N:2 * N], meta[2 * N:3 * N], meta[3 * N:]
    else:
        max_l = 0
        if not lx32.is_cuda:
            _validate_meta(lx32, None, None, T, V)
        lx_d = _h2d_async(lx32.cpu().reshape(-1), dev) if not lx32.is_cuda else lx32
        ly_d = off_d = lab_d = None
        meta = lx_d
    gh = _vp(graph) if (graph and c_den != 0.0) else _vp(0)
    ws_bytes = _lib.crf_workspace_bytes(gh, N, T, V, max_l)
    ws = _new_ws(ws_bytes, dev)
    if grad_out is not None:
        assert grad_out.shape == logits.shape and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad_out.device == dev
        grad = grad_out
    else:
        grad = torch.empty(logits.shape, dtype=torch.float32, device=dev)
    out = torch.empty(1 + 3 * N, dtype=torch.float32, device=dev)
    invalid = torch.empty(N, dtype=torch.int32, device=dev) if c_ctc != 0.0 else None
    loss, c_alpha, c_beta, c_ctc_t = out[:1], out[1:1 + N], out[1 + N:1 + 2 * N], out[1 + 2 * N:]
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if fused and c_den == 0.0:   # plain CTC on raw network output, either layout, any blank
            rc = _lib.crf_ctc_fwd_bwd_logits(_ptr(logits), _FUSED_DTYPES[logits.dtype], 1 if time_major else 0, blank, _ptr(lab_d), _ptr(off_d),
                                             _ptr(lx_d), _ptr(ly_d), N, T, V, max_l, c_ctc, _ptr(grad), _ptr(loss), _ptr(c_ctc_t),
                                             _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream))
        elif fused:
            rc = _lib.crf_loss_fwd_bwd_logits(gh, _ptr(logits), _FUSED_DTYPES[logits.dtype], _ptr(lab_d), _ptr(off_d), _ptr(lx_d),
                                              _ptr(ly_d), N, T, V, max_l, c_den, c_ctc, _ptr(grad), _ptr(loss), _ptr(c_alpha),
                                              _ptr(c_beta), _ptr(c_ctc_t), _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream))
        elif c_den == 0.0:   # numerator only: the layout and blank options (crf_loss_fwd_bwd's arguments, c_den = 0, in the default layout)
            rc = _lib.crf_ctc_fwd_bwd(_ptr(logits), 1 if time_major else 0, blank, _ptr(lab_d), _ptr(off_d), _ptr(lx_d), _ptr(ly_d),
                                      N, T, V, max_l, c_ctc, _ptr(grad), _ptr(loss), _ptr(c_ctc_t), _ptr(invalid), _ptr(ws), ws_bytes,
                                      _vp(stream))
        else:
            rc = _lib.crf_loss_fwd_bwd(gh, _ptr(logits), _ptr(lab_d), _ptr(off_d), _ptr(lx_d), _ptr(ly_d),
                                       N, T, V, max_l, c_den, c_ctc, _ptr(grad), _ptr(loss), _ptr(c_alpha),
                                       _ptr(c_beta), _ptr(c_ctc_t), _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream))
    _check(rc)
    if c_den != 0.0 and c_ctc != 0.0:
        _warn_if_serial((dev.index, int(stream)))
    del meta
    extras = dict(costs_alpha=c_alpha, costs_beta=c_beta, costs_ctc=c_ctc_t, invalid=invalid) if want_costs else {}
    return loss, grad, extras


def ctc_align(log_probs: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int = 0,
              time_major: bool = False, pos_out: Optional[torch.Tensor] = None, scores_out: Optional[torch.Tensor] = None,
              fused: bool = False):
    """Forced alignment (include/ctc_crf_hip.h ``crf_ctc_align``): the best path of every transcript through its 2L+1 states.

    log_probs [N,T,V] (time_major: [T,N,V]) f32 on the GPU, contiguous, read in place; labels / lx / ly int tensors on the CPU,
    labels flattened as for WARP_CTC_LOSS.  Returns (pos [N,T] int32, tokens [N,T] int32, scores [N] f32, invalid [N] int32), all on
    the device, no host synchronisation: pos = transcript index per frame, -1 for a blank frame, -2 past lx; tokens = the class emitted
    per frame (the blank's index where pos == -1, -1 where pos == -2), ONE gather of pos into a per-utterance table that travels with
    the staged metadata.  pos_out / scores_out: contiguous int32 [N,T] / f32 [N] device tensors that receive the results (else allocated).
    fused: log_probs is the RAW network output in f32 / bf16 / f16 (``crf_ctc_align_logits``): the path is the best one on the upcast
    values, the scores are those of log_softmax (the frames' normalisers subtracted in fp64)."""
    assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dim() == 3
    dev, N, T, V = _act_shape(log_probs, fused, time_major, blank)
    if labels.is_cuda or lx.is_cuda or ly.is_cuda:
        raise RuntimeError("ctc_align: labels, input_lengths and label_lengths are CPU tensors")
    lx32 = lx.to(torch.int32).reshape(-1)
    ly32 = ly.to(torch.int32).reshape(-1)
    lab32 = labels.to(torch.int32).reshape(-1)
    if lx32.numel() != N or ly32.numel() != N:
        raise RuntimeError(f"ctc_align: expect {N} input lengths and label lengths, got {lx32.numel()} and {ly32.numel()}")
    _validate_meta(lx32, ly32, lab32, T, V, blank)
    max_l = int(ly32.max()) if N > 0 else 0
    nlab = int(ly32.sum())
    off = (torch.cumsum(ly32, 0, dtype=torch.int32) - ly32).to(torch.int32)
    # tokens = table[n][pos + 2]: column 0 for pos = -2, column 1 the blank, then the transcript
    table = torch.full((N, max_l + 2), -1, dtype=torch.int32)
    table[:, 1] = blank
    table[:, 2:][torch.arange(max_l)[None, :] < ly32[:, None]] = lab32[:nlab]
    lab_pad = lab32[:nlab] if nlab else torch.zeros(1, dtype=torch.int32)
    meta = _h2d_async(torch.cat([lx32, ly32, off, table.reshape(-1), lab_pad]), dev)
    nt = N * (max_l + 2)
    lx_d, ly_d, off_d, table_d, lab_d = meta[:N], meta[N:2 * N], meta[2 * N:3 * N], meta[3 * N:3 * N + nt], meta[3 * N + nt:]
    ws_bytes = (_lib.crf_ctc_align_logits_workspace_bytes if fused else _lib.crf_ctc_align_workspace_bytes)(N, T, V, max_l)
    ws = _new_ws(ws_bytes, dev)
    pos = torch.empty((N, T), dtype=torch.int32, device=dev) if pos_out is None else pos_out
    scores = torch.empty(N, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert pos.shape == (N, T) and pos.dtype == torch.int32 and pos.is_contiguous() and pos.device == dev
    assert scores.shape == (N,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(N, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if fused:
            rc = _lib.crf_ctc_align_logits(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, blank, _ptr(lab_d),
                                           _ptr(off_d), _ptr(lx_d), _ptr(ly_d), N, T, V, max_l, _ptr(pos), _ptr(scores), _ptr(invalid),
                                           _ptr(ws), ws_bytes, _vp(stream))
        else:
            rc = _lib.crf_ctc_align(_ptr(log_probs), 1 if time_major else 0, blank, _ptr(lab_d), _ptr(off_d), _ptr(lx_d), _ptr(ly_d),
                                    N, T, V, max_l, _ptr(pos), _ptr(scores), _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream))
    _check(rc)
    tokens = torch.gather(table_d.view(N, max_l + 2), 1, (pos + 2).long())
    del meta
    return pos, tokens, scores, invalid


def _stage_score_meta(hyps: torch.Tensor, hyp_lengths: torch.Tensor, lx: torch.Tensor, hyp_utt: Optional[torch.Tensor], N: int, T: int,
                      V: int, blank: int):
    """The integer metadata of ctc_score as ONE int32 CPU tensor [lx (N) | hyp_len (H) | hyp_off (H) | hyp_utt (H) | labels], checked on
    the host; hyps flat [sum(hyp_lengths)] or padded (H, Lmax) -- both forms stage the same words.  Returns (meta, H, max_len)."""
    if hyps.is_cuda or hyp_lengths.is_cuda or lx.is_cuda or (hyp_utt is not None and hyp_utt.is_cuda):
        raise RuntimeError("ctc_score: hyps, hyp_lengths, input_lengths and hyp_utt are CPU tensors")
    lx32 = lx.to(torch.int32).reshape(-1)
    hl32 = hyp_lengths.to(torch.int32).reshape(-1)
    H = hl32.numel()
    if lx32.numel() != N:
        raise RuntimeError(f"ctc_score: expect {N} input lengths, got {lx32.numel()}")
    if H == 0:
        raise RuntimeError("ctc_score: no hypotheses")
    if hyp_utt is None:
        if H != N:
            raise RuntimeError(f"ctc_score: hyp_utt=None scores hypothesis h on utterance h: expect {N} hypotheses, got {H}")
        hu32 = torch.arange(N, dtype=torch.int32)
    else:
        hu32 = hyp_utt.to(torch.int32).reshape(-1)
        if hu32.numel() != H:
            raise RuntimeError(f"ctc_score: expect {H} entries of hyp_utt (one per hypothesis), got {hu32.numel()}")
        if int(hu32.min()) < 0 or int(hu32.max()) >= N:
            raise RuntimeError(f"ctc_score: hyp_utt must lie in [0, N-1={N - 1}], got [{int(hu32.min())}, {int(hu32.max())}]")
    if int(hl32.min()) < 0:
        raise RuntimeError("negative label length")
    max_l = int(hl32.max())
    if hyps.dim() == 2:   # padded rows: the first hyp_lengths[h] entries of row h
        if hyps.size(0) != H:
            raise RuntimeError(f"ctc_score: expect {H} rows of hyps (one per hypothesis), got {hyps.size(0)}")
        if max_l > hyps.size(1):
            raise RuntimeError(f"ctc_score: max(hyp_lengths)={max_l} exceeds the row length {hyps.size(1)} of hyps")
        lab32 = hyps.to(torch.int32)[torch.arange(hyps.size(1))[None, :] < hl32[:, None]]
    else:
        lab32 = hyps.to(torch.int32).reshape(-1)
    _validate_meta(lx32, hl32, lab32, T, V, blank)
    nlab = int(hl32.sum())
    off = (torch.cumsum(hl32, 0, dtype=torch.int32) - hl32).to(torch.int32)
    lab_pad = lab32[:nlab] if nlab else torch.zeros(1, dtype=torch.int32)
    return torch.cat([lx32, hl32, off, hu32, lab_pad]), H, max_l


def ctc_score(log_probs: torch.Tensor, hyps: torch.Tensor, hyp_lengths: torch.Tensor, lx: torch.Tensor,
              hyp_utt: Optional[torch.Tensor] = None, blank: int = 0, time_major: bool = False, fused: bool = False,
              scores_out: Optional[torch.Tensor] = None, max_hyp_len: Optional[int] = None):
    """Forward-only CTC log-likelihoods of H hypotheses (include/ctc_crf_hip.h ``crf_ctc_score``): hypothesis h on the rows of utterance
    hyp_utt[h] (None: H = N, hypothesis h on utterance h).  hyps on the device: padded rows as stage_score_rows takes them, scored where
    they lie by ``crf_ctc_score_rows`` with the bound max_hyp_len; a hypothesis over the bound comes back invalid with -inf.

    log_probs [N,T,V] (time_major: [T,N,V]) f32 on the GPU, contiguous, read in place and never replicated; hyps / hyp_lengths / lx /
    hyp_utt int tensors on the CPU, hyps flat [sum(hyp_lengths)] or padded (H, Lmax).  Returns (scores [H] f32 = +log p, invalid [H]
    int32), both on the device, no host synchronisation, no autograd; all integer metadata travels in one staged copy.
    fused: log_probs is the RAW network output in f32 / bf16 / f16 (``crf_ctc_score_logits``)."""
    assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dim() == 3
    if device_rows("ctc_score", hyps, hyp_lengths, hyp_utt, max_hyp_len):
        sr = stage_score_rows(log_probs, hyps, hyp_lengths, lx, hyp_utt, blank, time_major, fused, max_hyp_len)
        return _ctc_score_rows(log_probs, sr, time_major, scores_out, fused)
    dev, N, T, V = _act_shape(log_probs, fused, time_major, blank)
    meta_cpu, H, max_l = _stage_score_meta(hyps, hyp_lengths, lx, hyp_utt, N, T, V, blank)
    meta = _h2d_async(meta_cpu, dev)
    lx_d, len_d, off_d, utt_d, lab_d = meta[:N], meta[N:N + H], meta[N + H:N + 2 * H], meta[N + 2 * H:N + 3 * H], meta[N + 3 * H:]
    scores = torch.empty(H, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert scores.shape == (H,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(H, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if fused:
            ws_bytes = _lib.crf_ctc_score_logits_workspace_bytes(N, T, V)
            ws = _new_ws(ws_bytes, dev)
            rc = _lib.crf_ctc_score_logits(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, blank, _ptr(lab_d),
                                           _ptr(off_d), _ptr(len_d), _ptr(utt_d), _ptr(lx_d), N, H, T, V, max_l, _ptr(scores),
                                           _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream))
        else:
            rc = _lib.crf_ctc_score(_ptr(log_probs), 1 if time_major else 0, blank, _ptr(lab_d), _ptr(off_d), _ptr(len_d), _ptr(utt_d),
                                    _ptr(lx_d), N, H, T, V, max_l, _ptr(scores), _ptr(invalid), _vp(stream))
    _check(rc)
    del meta
    return scores, invalid


SCORE_GRAD_MAX_LEN = 255     # longest hypothesis crf_ctc_score_grad takes (one wave per hypothesis; include/ctc_crf_hip.h)


class ScoreMeta:
    """The staged integer metadata of one list of hypotheses, on the device: what ctc_score_staged and ctc_score_grad share, so that a
    backward pass needs no second host-to-device copy.  `meta` = [lx (N) | hyp_len (H) | hyp_off (H) | hyp_utt (H) | labels] int32."""

    def __init__(self, meta: torch.Tensor, N: int, H: int, T: int, V: int, max_len: int, blank: int):
        self.meta, self.N, self.H, self.T, self.V, self.max_len, self.blank = meta, N, H, T, V, max_len, blank

    def parts(self):
        m, N, H = self.meta, self.N, self.H
        return m[:N], m[N:N + H], m[N + H:N + 2 * H], m[N + 2 * H:N + 3 * H], m[N + 3 * H:]   # lx, len, off, utt, labels


def stage_score_meta(log_probs: torch.Tensor, hyps: torch.Tensor, hyp_lengths: torch.Tensor, lx: torch.Tensor,
                     hyp_utt: Optional[torch.Tensor], blank: int, time_major: bool, fused: bool = False) -> ScoreMeta:
    """_stage_score_meta's checks and ONE staged copy to log_probs' device (fp32 log-probs, as ctc_score takes them; fused: raw network
    output in f32 / bf16 / f16)."""
    assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dim() == 3
    dev, N, T, V = _act_shape(log_probs, fused, time_major, blank)
    meta_cpu, H, max_l = _stage_score_meta(hyps, hyp_lengths, lx, hyp_utt, N, T, V, blank)
    return ScoreMeta(_h2d_async(meta_cpu, dev), N, H, T, V, max_l, blank)


SCORE_ROWS_MAX_LEN = 2047    # longest hypothesis crf_ctc_score_rows takes (the workgroup geometry's eight states per thread)


class ScoreRows:
    """ScoreMeta's twin for hypotheses that lie on the device as padded rows (what ctc_sample, ctc_greedy and ctc_beam_search return):
    nothing of them is known on the host but the shapes and `len_cap`, the caller's bound on the lengths.  ctc_score_staged and
    ctc_score_grad take either; forward and backward of ctc_logp share one."""

    def __init__(self, hyps: torch.Tensor, hyp_len: torch.Tensor, hyp_utt: torch.Tensor, lx: torch.Tensor, N: int, H: int, T: int, V: int,
                 stride: int, len_cap: int, blank: int):
        self.hyps, self.hyp_len, self.hyp_utt, self.lx = hyps, hyp_len, hyp_utt, lx
        self.N, self.H, self.T, self.V, self.stride, self.len_cap, self.blank = N, H, T, V, stride, len_cap, blank
        self.meta = hyp_len          # (what _score_args checks the device of)


def device_rows(who: str, hyps, hyp_lengths, hyp_utt, max_hyp_len) -> bool:
    """True: the hypotheses are device rows.  A mix of CPU and CUDA tensors among hyps / hyp_lengths / hyp_utt, and max_hyp_len with CPU
    hypotheses, raise -- from the tensors' placement alone, before anything touches a device."""
    named = [("hyps", hyps), ("hyp_lengths", hyp_lengths)] + ([("hyp_utt", hyp_utt)] if hyp_utt is not None else [])
    for name, t in named[1:]:
        if t.is_cuda != hyps.is_cuda:
            raise RuntimeError(f"{who}: {name} is a {'CUDA' if t.is_cuda else 'CPU'} tensor, hyps a {'CUDA' if hyps.is_cuda else 'CPU'} tensor: "
                               "hypotheses lie on one side, all on the CPU or all on log_probs' device")
    if not hyps.is_cuda and max_hyp_len is not None:
        raise RuntimeError(f"{who}: max_hyp_len bounds hypotheses that lie on the device; with CPU hypotheses the host knows the lengths, "
                           "pass None")
    return hyps.is_cuda


def stage_score_rows(log_probs: torch.Tensor, hyps: torch.Tensor, hyp_lengths: torch.Tensor, lx: torch.Tensor,
                     hyp_utt: Optional[torch.Tensor], blank: int, time_major: bool, fused: bool = False, max_hyp_len: Optional[int] = None,
                     grad: bool = False, who: str = "ctc_score") -> ScoreRows:
    """The checks of device rows -- shapes, dtypes and placement only: NO value of a device tensor is read on the host (no .max(), .item(),
    .cpu(), int(tensor) or truth test of a tensor) -- and the staged copy of CPU input lengths.  hyps (H, W) int32 with contiguous rows,
    hyp_lengths (H,) int32, hyp_utt (H,) int32 or None (H = N, an arange built on the device), all on log_probs' device; lx on the CPU
    (staged without a synchronisation) or on the device.  max_hyp_len: the bound len_cap, default min(W, 2047) -- grad: min(W, 255)."""
    assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dim() == 3
    dev, N, T, V = _act_shape(log_probs, fused, time_major, blank)
    if hyps.dim() != 2 or hyps.dtype != torch.int32:
        raise RuntimeError(f"{who}: device hyps are padded rows (H, W) of int32, got {tuple(hyps.shape)} of {hyps.dtype}")
    H, W = hyps.shape
    if H == 0 or W == 0:
        raise RuntimeError(f"{who}: no hypotheses")
    if W > 1 and hyps.stride(1) != 1 or H > 1 and hyps.stride(0) < W:
        raise RuntimeError(f"{who}: the rows of device hyps must be contiguous, got strides {tuple(hyps.stride())}")
    stride = hyps.stride(0) if H > 1 else W
    for name, t in (("hyp_lengths", hyp_lengths), ("hyp_utt", hyp_utt)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (H,) or not t.is_contiguous()):
            raise RuntimeError(f"{who}: expect {name} as a contiguous int32 tensor ({H},) (one entry per row of hyps), got {tuple(t.shape)} of {t.dtype}")
    for name, t in (("hyps", hyps), ("hyp_lengths", hyp_lengths), ("hyp_utt", hyp_utt)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{who}: {name} lies on {t.device}, log_probs on {dev}")
    if H * stride > 2 ** 31 - 1:
        raise RuntimeError(f"{who}: H * row stride = {H * stride} exceeds INT32_MAX")
    limit = SCORE_GRAD_MAX_LEN if grad else SCORE_ROWS_MAX_LEN
    if max_hyp_len is None:
        len_cap = min(W, limit)
    else:
        if isinstance(max_hyp_len, bool) or not isinstance(max_hyp_len, int) or max_hyp_len < 0:
            raise RuntimeError(f"{who}: max_hyp_len must be a non-negative int or None, got {max_hyp_len!r}")
        if max_hyp_len > limit:
            raise RuntimeError(f"{who}: max_hyp_len={max_hyp_len} exceeds {limit}, the longest hypothesis "
                               + ("the gradient takes" if grad else "the score kernels take"))
        len_cap = max_hyp_len
    if lx.is_cuda:
        if lx.dtype != torch.int32 or lx.shape != (N,) or not lx.is_contiguous() or lx.device != dev:
            raise RuntimeError(f"{who}: device input_lengths must be a contiguous int32 tensor ({N},) on {dev}, got {tuple(lx.shape)} of {lx.dtype} on {lx.device}")
        lx_d = lx
    else:
        lx32 = lx.to(torch.int32).reshape(-1)
        if lx32.numel() != N:
            raise RuntimeError(f"{who}: expect {N} input lengths, got {lx32.numel()}")
        _validate_meta(lx32, None, None, T, V, blank)
        lx_d = _h2d_async(lx32, dev)
    if hyp_utt is None:
        if H != N:
            raise RuntimeError(f"{who}: hyp_utt=None scores hypothesis h on utterance h: expect {N} hypotheses, got {H}")
        hyp_utt = torch.arange(N, dtype=torch.int32, device=dev)
    return ScoreRows(hyps, hyp_lengths, hyp_utt, lx_d, N, H, T, V, stride, len_cap, blank)


def _rows_dtype(log_probs: torch.Tensor, fused: bool) -> int:
    return _FUSED_DTYPES[log_probs.dtype] if fused else -1


def _ctc_score_rows(log_probs: torch.Tensor, sr: ScoreRows, time_major: bool, scores_out: Optional[torch.Tensor], fused: bool):
    """crf_ctc_score_rows on staged device rows -> (scores [H] f32, invalid [H] int32)."""
    dev, N, T, V = _score_args(log_probs, sr, time_major, fused)
    dtype = _rows_dtype(log_probs, fused)
    scores = torch.empty(sr.H, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert scores.shape == (sr.H,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(sr.H, dtype=torch.int32, device=dev)
    ws_bytes = _lib.crf_ctc_score_rows_workspace_bytes(N, sr.H, T, V, sr.len_cap, dtype)
    ws = _new_ws(ws_bytes, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _check(_lib.crf_ctc_score_rows(_ptr(log_probs), dtype, 1 if time_major else 0, sr.blank, _ptr(sr.hyps), sr.stride, _ptr(sr.hyp_len),
                                       _ptr(sr.hyp_utt), _ptr(sr.lx), N, sr.H, T, V, sr.len_cap, _ptr(scores), _ptr(invalid), _ptr(ws), ws_bytes,
                                       _vp(stream)))
    return scores, invalid


def _ctc_score_grad_rows(log_probs: torch.Tensor, sr: ScoreRows, weights: Optional[torch.Tensor], time_major: bool,
                         grad_out: Optional[torch.Tensor], scores_out: Optional[torch.Tensor], fused: bool):
    """crf_ctc_score_grad_rows on staged device rows -> (grad, scores [H] f32, invalid [H] int32)."""
    dev, N, T, V = _score_args(log_probs, sr, time_major, fused)
    dtype, H = _rows_dtype(log_probs, fused), sr.H
    if sr.len_cap > SCORE_GRAD_MAX_LEN:
        raise RuntimeError(f"ctc_score_grad: max_hyp_len={sr.len_cap} exceeds {SCORE_GRAD_MAX_LEN}, the longest hypothesis the gradient takes")
    if weights is not None:
        assert weights.shape == (H,) and weights.dtype == torch.float32 and weights.is_contiguous() and weights.device == dev
    ws_bytes = _lib.crf_ctc_score_grad_rows_workspace_bytes(N, H, T, V, sr.len_cap, dtype)
    ws = _new_ws(ws_bytes, dev)
    grad = torch.empty(log_probs.shape, dtype=torch.float32, device=dev) if grad_out is None else grad_out
    assert grad.shape == log_probs.shape and grad.dtype == torch.float32 and grad.is_contiguous() and grad.device == dev
    scores = torch.empty(H, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert scores.shape == (H,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(H, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _check(_lib.crf_ctc_score_grad_rows(_ptr(log_probs), dtype, 1 if time_major else 0, sr.blank, _ptr(sr.hyps), sr.stride, _ptr(sr.hyp_len),
                                            _ptr(sr.hyp_utt), _ptr(sr.lx), _ptr(weights), N, H, T, V, sr.len_cap, _ptr(scores), _ptr(invalid),
                                            _ptr(grad), _ptr(ws), ws_bytes, _vp(stream)))
    return grad, scores, invalid


def _score_args(log_probs: torch.Tensor, sm: ScoreMeta, time_major: bool, fused: bool = False):
    dev, N, T, V = _act_shape(log_probs, fused, time_major, sm.blank)
    assert log_probs.is_cuda and log_probs.is_contiguous() and (N, T, V) == (sm.N, sm.T, sm.V) and sm.meta.device == dev
    return dev, N, T, V


def ctc_score_staged(log_probs: torch.Tensor, sm: ScoreMeta, time_major: bool = False, scores_out: Optional[torch.Tensor] = None,
                     fused: bool = False):
    """ctc_score's crf_ctc_score call (fused: its crf_ctc_score_logits call, on raw network output in f32 / bf16 / f16) on metadata that is
    staged already (a ScoreRows: crf_ctc_score_rows on device rows).  Returns (scores [H] f32, invalid [H] int32)."""
    if isinstance(sm, ScoreRows):
        return _ctc_score_rows(log_probs, sm, time_major, scores_out, fused)
    dev, N, T, V = _score_args(log_probs, sm, time_major, fused)
    lx_d, len_d, off_d, utt_d, lab_d = sm.parts()
    scores = torch.empty(sm.H, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert scores.shape == (sm.H,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(sm.H, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if fused:
            ws_bytes = _lib.crf_ctc_score_logits_workspace_bytes(N, T, V)
            ws = _new_ws(ws_bytes, dev)
            _check(_lib.crf_ctc_score_logits(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, sm.blank, _ptr(lab_d),
                                             _ptr(off_d), _ptr(len_d), _ptr(utt_d), _ptr(lx_d), N, sm.H, T, V, sm.max_len, _ptr(scores),
                                             _ptr(invalid), _ptr(ws), ws_bytes, _vp(stream)))
        else:
            _check(_lib.crf_ctc_score(_ptr(log_probs), 1 if time_major else 0, sm.blank, _ptr(lab_d), _ptr(off_d), _ptr(len_d), _ptr(utt_d),
                                      _ptr(lx_d), N, sm.H, T, V, sm.max_len, _ptr(scores), _ptr(invalid), _vp(stream)))
    return scores, invalid


def ctc_score_grad(log_probs: torch.Tensor, meta, weights: Optional[torch.Tensor], blank: int = 0, time_major: bool = False,
                   grad_out: Optional[torch.Tensor] = None, scores_out: Optional[torch.Tensor] = None, fused: bool = False):
    """The weighted gradient of the hypothesis scores as ONE tensor of log_probs' shape (include/ctc_crf_hip.h ``crf_ctc_score_grad``):
    grad[u] = sum over the hypotheses h of utterance u of weights[h] * d score[h] / d log_probs[u].
    fused: log_probs is the RAW network output in f32 / bf16 / f16 (``crf_ctc_score_grad_logits``): scores and invalid are
    ctc_score(fused=True)'s bits, the gradient (f32) is the one with respect to the raw output, log_softmax's backward included.

    log_probs [N,T,V] (time_major: [T,N,V]) f32 log-probs on the GPU, contiguous, read in place and never replicated; meta: a ScoreMeta
    (stage_score_meta; its blank counts) or the tuple (hyps, hyp_lengths, input_lengths, hyp_utt) of CPU tensors as ctc_score takes them;
    weights: [H] f32 on the device, or None for all 1.  Returns (grad, scores [H] f32, invalid [H] int32), all on the device, no host
    synchronisation; scores and invalid are ctc_score's bits.  grad_out / scores_out: contiguous f32 device tensors of log_probs' shape /
    [H] that receive the results (else allocated); every entry of grad is written."""
    assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dim() == 3
    if isinstance(meta, ScoreRows):            # device rows: crf_ctc_score_grad_rows, the workspace sized by the bound meta.len_cap
        return _ctc_score_grad_rows(log_probs, meta, weights, time_major, grad_out, scores_out, fused)
    sm = meta if isinstance(meta, ScoreMeta) else stage_score_meta(log_probs, *meta, blank, time_major, fused)
    dev, N, T, V = _score_args(log_probs, sm, time_major, fused)
    H = sm.H
    lx_d, len_d, off_d, utt_d, lab_d = sm.parts()
    if weights is not None:
        assert weights.shape == (H,) and weights.dtype == torch.float32 and weights.is_contiguous() and weights.device == dev
    ws_bytes = (_lib.crf_ctc_score_grad_logits_workspace_bytes if fused else _lib.crf_ctc_score_grad_workspace_bytes)(N, H, T, V, sm.max_len)
    ws = _new_ws(ws_bytes, dev)
    grad = torch.empty(log_probs.shape, dtype=torch.float32, device=dev) if grad_out is None else grad_out
    assert grad.shape == log_probs.shape and grad.dtype == torch.float32 and grad.is_contiguous() and grad.device == dev
    scores = torch.empty(H, dtype=torch.float32, device=dev) if scores_out is None else scores_out
    assert scores.shape == (H,) and scores.dtype == torch.float32 and scores.is_contiguous() and scores.device == dev
    invalid = torch.empty(H, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if fused:
            rc = _lib.crf_ctc_score_grad_logits(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, sm.blank, _ptr(lab_d),
                                                _ptr(off_d), _ptr(len_d), _ptr(utt_d), _ptr(lx_d), _ptr(weights), N, H, T, V, sm.max_len,
                                                _ptr(scores), _ptr(invalid), _ptr(grad), _ptr(ws), ws_bytes, _vp(stream))
        else:
            rc = _lib.crf_ctc_score_grad(_ptr(log_probs), 1 if time_major else 0, sm.blank, _ptr(lab_d), _ptr(off_d), _ptr(len_d), _ptr(utt_d),
                                         _ptr(lx_d), _ptr(weights), N, H, T, V, sm.max_len, _ptr(scores), _ptr(invalid), _ptr(grad), _ptr(ws),
                                         ws_bytes, _vp(stream))
    _check(rc)
    return grad, scores, invalid


def ctc_sample(log_probs: torch.Tensor, lx: torch.Tensor, n_samples: int, seed: int, offset: int = 0, blank: int = 0,
               time_major: bool = False, greedy: bool = False, return_paths: bool = False, hyps_out: Optional[torch.Tensor] = None,
               paths_out: Optional[torch.Tensor] = None):
    """Label sequences drawn on the GPU (include/ctc_crf_hip.h ``crf_ctc_sample``): per frame K = n_samples classes from
    softmax(log_probs) -- counter-based, Philox4x32-10 on (seed, offset, n, t, k) -- or with greedy the arg-max (K = 1), then the CTC
    collapse of each of the N K frame paths.

    log_probs [N,T,V] (time_major: [T,N,V]) f32 / bf16 / f16 on the GPU, contiguous, read in place; lx an int tensor on the CPU.  Returns
    (hyps [N K, T] int32, padded with the blank's index; hyp_lengths [N K] int32; paths [N K, T] int32 or None: the class per frame, -1
    past lx), all on the device, no host synchronisation.  hyps_out / paths_out: contiguous int32 [N K, T] device tensors that receive
    the results (else allocated; paths_out implies return_paths)."""
    who = "ctc_greedy" if greedy else "ctc_sample"
    if log_probs.dtype not in _FUSED_DTYPES:
        raise RuntimeError(f"{who}: expect float32, bfloat16 or float16 activations, got {log_probs.dtype}")
    if log_probs.dim() != 3:
        raise RuntimeError(f"{who}: expect (N, T, V) or (T, N, V) activations, got {log_probs.dim()} dimensions")
    N, T, V = _check_sample_args(log_probs.shape, lx, n_samples, seed, offset, blank, time_major, greedy)
    if not log_probs.is_cuda:                  # (after the checks of the arguments: those need no device)
        raise RuntimeError(f"{who}: log_probs must be on the GPU (there is no CPU path)")
    assert log_probs.is_contiguous()
    K = int(n_samples)
    dev = log_probs.device
    lx_d = _h2d_async(lx.to(torch.int32).reshape(-1), dev)
    H = N * K
    ws_bytes = _lib.crf_ctc_sample_workspace_bytes(N, T, V, K)
    ws = _new_ws(ws_bytes, dev)
    hyps = torch.empty((H, T), dtype=torch.int32, device=dev) if hyps_out is None else hyps_out
    paths = paths_out if paths_out is not None else torch.empty((H, T), dtype=torch.int32, device=dev) if return_paths else None
    for o in (hyps, paths):
        assert o is None or (o.shape == (H, T) and o.dtype == torch.int32 and o.is_contiguous() and o.device == dev)
    hyp_len = torch.empty(H, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = _lib.crf_ctc_sample(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, int(blank), _ptr(lx_d), N, T, V, K,
                                 int(seed), int(offset), 1 if greedy else 0, _ptr(hyps), _ptr(hyp_len), _ptr(paths), _ptr(ws), ws_bytes,
                                 _vp(stream))
    _check(rc)
    del lx_d
    return hyps, hyp_len, paths


def _check_sample_args(shape, lx: torch.Tensor, n_samples: int, seed: int, offset: int, blank: int, time_major: bool, greedy: bool):
    """The host checks of ctc_sample / ctc_greedy, each with the offending value in the message.  -> (N, T, V)."""
    who = "ctc_greedy" if greedy else "ctc_sample"
    N, T, V = shape
    if time_major:
        T, N = N, T
    if not 0 <= blank < V:
        raise RuntimeError(f"blank must lie in [0, V-1={V - 1}], got {blank}")
    if int(n_samples) < 1:
        raise RuntimeError(f"{who}: n_samples must be at least 1, got {n_samples}")
    if greedy and int(n_samples) != 1:
        raise RuntimeError(f"{who}: the best path is one path per utterance, got n_samples={n_samples}")
    if not 0 <= int(seed) < 1 << 64:
        raise RuntimeError(f"{who}: seed must lie in [0, 2^64), got {seed}")
    if not 0 <= int(offset) < 1 << 32:
        raise RuntimeError(f"{who}: offset must lie in [0, 2^32), got {offset}")
    if lx.is_cuda:
        raise RuntimeError(f"{who}: input_lengths is a CPU tensor")
    lx32 = lx.to(torch.int32).reshape(-1)
    if lx32.numel() != N:
        raise RuntimeError(f"{who}: expect {N} input lengths, got {lx32.numel()}")
    if N > 0 and int(lx32.max()) > T:
        raise RuntimeError(f"frame lengths must lie in [0, T={T}], got max {int(lx32.max())}")
    return N, T, V


BEAM_MAX_WIDTH = 64          # widest beam and most classes per frame crf_ctc_beam takes (one lane each; include/ctc_crf_hip.h)
BEAM_MAX_CLASSES = 64


def _check_beam_args(shape, lx: torch.Tensor, beam_size: int, nbest: int, top_classes: int, blank: int, time_major: bool):
    """The host checks of ctc_beam_search, each with the offending value in the message.  -> (N, T, V)."""
    who = "ctc_beam_search"
    N, T, V = shape
    if time_major:
        T, N = N, T
    if not 0 <= blank < V:
        raise RuntimeError(f"blank must lie in [0, V-1={V - 1}], got {blank}")
    if not 1 <= int(beam_size) <= BEAM_MAX_WIDTH:
        raise RuntimeError(f"{who}: beam_size must lie in [1, {BEAM_MAX_WIDTH}], got {beam_size}")
    if not 1 <= int(nbest) <= int(beam_size):
        raise RuntimeError(f"{who}: nbest must lie in [1, beam_size={beam_size}], got {nbest}")
    if not 1 <= int(top_classes) <= BEAM_MAX_CLASSES:
        raise RuntimeError(f"{who}: top_classes must lie in [1, {BEAM_MAX_CLASSES}], got {top_classes}")
    if lx.is_cuda:
        raise RuntimeError(f"{who}: input_lengths is a CPU tensor")
    lx32 = lx.to(torch.int32).reshape(-1)
    if lx32.numel() != N:
        raise RuntimeError(f"{who}: expect {N} input lengths, got {lx32.numel()}")
    if N > 0 and int(lx32.max()) > T:
        raise RuntimeError(f"frame lengths must lie in [0, T={T}], got max {int(lx32.max())}")
    return N, T, V


def _check_beam_lm_args(lm, alpha, beta, return_lm_scores, V: int):
    """The host checks of ctc_beam_search's LM arguments, each with the offending value in the message; none needs a device."""
    import math
    import numbers
    from ..ngram_lm import NgramLM
    who = "ctc_beam_search"
    for name, v in (("alpha", alpha), ("beta", beta)):
        if not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise RuntimeError(f"{who}: {name} must be a finite number, got {v!r}")
    if lm is None:
        if alpha != 0 or beta != 0:
            raise RuntimeError(f"{who}: alpha and beta weigh a language model: without lm they must be 0, got alpha={alpha!r}, beta={beta!r}")
        if return_lm_scores:
            raise RuntimeError(f"{who}: return_lm_scores needs lm")
        return
    if not isinstance(lm, NgramLM):
        raise RuntimeError(f"{who}: lm must be an NgramLM (cat_amd.ngram_lm), got {type(lm).__name__}: {lm!r}")
    if lm.vocab_size != V:
        raise RuntimeError(f"{who}: the LM is over {lm.vocab_size} classes, the activations have V={V}")


def ctc_beam_search(log_probs: torch.Tensor, lx: torch.Tensor, beam_size: int = 16, nbest: int = 1, top_classes: int = 40, blank: int = 0,
                    time_major: bool = False, fused: bool = False, return_trace: bool = False, lm=None, alpha: float = 0.0, beta: float = 0.0,
                    return_lm_scores: bool = False):
    """CTC prefix beam search on the GPU (include/ctc_crf_hip.h ``crf_ctc_beam``): the nbest best label sequences of every utterance among
    a beam of beam_size prefixes, per frame the blank and the top_classes classes of largest value.  With lm (a cat_amd.ngram_lm.NgramLM)
    the search is ``crf_ctc_beam_lm``'s: scores are fused, score + alpha log P_lm + beta length, and with return_lm_scores the LM part is
    returned behind the trace (else None); the tables are uploaded once per device and kept.

    log_probs [N,T,V] (time_major: [T,N,V]) f32 / bf16 / f16 on the GPU, contiguous, read in place: log-probs, or with fused the RAW
    network output (log_softmax of the upcast values inside the call); lx an int tensor on the CPU.  Returns (hyps [N nbest, T] int32,
    padded with the blank's index; hyp_lengths [N nbest] int32; scores [N nbest] f32, -inf for a missing rank; trace [N, T, beam_size]
    int32 or None), all on the device, no host synchronisation."""
    who = "ctc_beam_search"
    if log_probs.dtype not in _FUSED_DTYPES:
        raise RuntimeError(f"{who}: expect float32, bfloat16 or float16 activations, got {log_probs.dtype}")
    if log_probs.dim() != 3:
        raise RuntimeError(f"{who}: expect (N, T, V) or (T, N, V) activations, got {log_probs.dim()} dimensions")
    N, T, V = _check_beam_args(log_probs.shape, lx, beam_size, nbest, top_classes, blank, time_major)
    _check_beam_lm_args(lm, alpha, beta, return_lm_scores, V)
    if not log_probs.is_cuda:                  # (after the checks of the arguments: those need no device)
        raise RuntimeError(f"{who}: log_probs must be on the GPU (there is no CPU path)")
    assert log_probs.is_contiguous()
    W, K, C = int(beam_size), int(nbest), int(top_classes)
    dev = log_probs.device
    lx_d = _h2d_async(lx.to(torch.int32).reshape(-1), dev)
    H = N * K
    ws_bytes = _lib.crf_ctc_beam_workspace_bytes(N, T, V, W, C)
    ws = _new_ws(ws_bytes, dev)
    hyps = torch.empty((H, T), dtype=torch.int32, device=dev)
    hyp_len = torch.empty(H, dtype=torch.int32, device=dev)
    scores = torch.empty(H, dtype=torch.float32, device=dev)
    trace = torch.empty((N, T, W), dtype=torch.int32, device=dev) if return_trace else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    if lm is not None:
        tables, _keep = lm.tables(dev)
        lm_scores = torch.empty(H, dtype=torch.float32, device=dev) if return_lm_scores else None
        with torch.cuda.device(dev):
            rc = _lib.crf_ctc_beam_lm(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, int(blank), 1 if fused else 0,
                                      _ptr(lx_d), N, T, V, W, K, C, ctypes.byref(tables), float(alpha), float(beta), _ptr(hyps), _ptr(hyp_len),
                                      _ptr(scores), _ptr(lm_scores), _ptr(trace), _ptr(ws), ws_bytes, _vp(stream))
        _check(rc)
        del lx_d
        return hyps, hyp_len, scores, trace, lm_scores
    with torch.cuda.device(dev):
        rc = _lib.crf_ctc_beam(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, int(blank), 1 if fused else 0,
                               _ptr(lx_d), N, T, V, W, K, C, _ptr(hyps), _ptr(hyp_len), _ptr(scores), _ptr(trace), _ptr(ws), ws_bytes,
                               _vp(stream))
    _check(rc)
    del lx_d
    return hyps, hyp_len, scores, trace


BEAM_STATE_MAX_HYP_LEN = 8192   # most labels a BeamState keeps per prefix (include/ctc_crf_hip.h crf_ctc_beam_chunk: cap)


class BeamState:
    """The beams of N utterances between two ctc_beam_search_chunk calls: the (N, record_bytes) uint8 tensor of records that
    include/ctc_crf_hip.h ``crf_ctc_beam_chunk`` writes, and the values it was made under.  Immutable: every call allocates the records
    it returns, none writes to the records it continues from, so a state can be continued any number of times."""
    FIELDS = ("beam_size", "top_classes", "blank", "max_hyp_len", "lm", "alpha", "beta")
    __slots__ = ("records",) + FIELDS

    def __init__(self, records: torch.Tensor, beam_size: int, top_classes: int, blank: int, max_hyp_len: int, lm, alpha: float, beta: float):
        self.records = records
        self.beam_size, self.top_classes, self.blank, self.max_hyp_len = int(beam_size), int(top_classes), int(blank), int(max_hyp_len)
        self.lm, self.alpha, self.beta = lm, float(alpha), float(beta)

    def _like(self, records: torch.Tensor) -> "BeamState":
        return BeamState(records, self.beam_size, self.top_classes, self.blank, self.max_hyp_len, self.lm, self.alpha, self.beta)

    def __len__(self) -> int:
        return self.records.size(0)

    def index_select(self, index: torch.Tensor) -> "BeamState":
        """The states of the utterances index[0], index[1], ... (an int tensor; on the CPU it is copied to the records' device)."""
        return self._like(self.records.index_select(0, index.to(device=self.records.device, dtype=torch.int64)))

    def clone(self) -> "BeamState":
        return self._like(self.records.clone())

    def __repr__(self) -> str:
        return "BeamState(N=%d, %s)" % (len(self), ", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS))


def ctc_beam_search_chunk(log_probs: torch.Tensor, lx: torch.Tensor, state: Optional[BeamState] = None, reset: Optional[torch.Tensor] = None,
                          beam_size: int = 16, nbest: int = 1, top_classes: int = 40, blank: int = 0, time_major: bool = False,
                          fused: bool = False, lm=None, alpha: float = 0.0, beta: float = 0.0, max_hyp_len: int = 512,
                          return_trace: bool = False, return_lm_scores: bool = False):
    """ctc_beam_search on a chunk of frames, the beam carried in a BeamState (include/ctc_crf_hip.h ``crf_ctc_beam_chunk``).

    log_probs [N,Tc,V] (time_major: [Tc,N,V]) as for ctc_beam_search; lx (N,): the chunk's frames per utterance, an int tensor on the
    CPU (checked against [0, Tc]) or an int32 tensor on the GPU (used as is, clamped in the kernel); reset: None or (N,) bool / int, CPU
    or GPU.  Returns (BeamState, hyps [N nbest, max_hyp_len] int32, hyp_lengths, scores, trace [N, Tc, beam_size] or None, lm_scores or
    None), all on the device, no host synchronisation."""
    who = "ctc_beam_search_chunk"
    if log_probs.dtype not in _FUSED_DTYPES:
        raise RuntimeError(f"{who}: expect float32, bfloat16 or float16 activations, got {log_probs.dtype}")
    if log_probs.dim() != 3:
        raise RuntimeError(f"{who}: expect (N, Tc, V) or (Tc, N, V) activations, got {log_probs.dim()} dimensions")
    N, T, V = log_probs.shape
    if time_major:
        T, N = N, T
    if N < 1 or T < 1 or V < 1:
        raise RuntimeError(f"{who}: expect a chunk of at least one utterance, frame and class, got shape {tuple(log_probs.shape)}")
    if not 0 <= blank < V:
        raise RuntimeError(f"blank must lie in [0, V-1={V - 1}], got {blank}")
    if not 1 <= int(beam_size) <= BEAM_MAX_WIDTH:
        raise RuntimeError(f"{who}: beam_size must lie in [1, {BEAM_MAX_WIDTH}], got {beam_size}")
    if not 1 <= int(nbest) <= int(beam_size):
        raise RuntimeError(f"{who}: nbest must lie in [1, beam_size={beam_size}], got {nbest}")
    if not 1 <= int(top_classes) <= BEAM_MAX_CLASSES:
        raise RuntimeError(f"{who}: top_classes must lie in [1, {BEAM_MAX_CLASSES}], got {top_classes}")
    if not 1 <= int(max_hyp_len) <= BEAM_STATE_MAX_HYP_LEN:
        raise RuntimeError(f"{who}: max_hyp_len must lie in [1, {BEAM_STATE_MAX_HYP_LEN}], got {max_hyp_len}")
    if lx.dim() != 1 or lx.numel() != N:
        raise RuntimeError(f"{who}: expect {N} input lengths, got shape {tuple(lx.shape)}")
    if lx.is_cuda:
        if lx.dtype != torch.int32:
            raise RuntimeError(f"{who}: input_lengths on the GPU must be int32, got {lx.dtype}")
    else:
        if lx.dtype.is_floating_point or lx.dtype == torch.bool:
            raise RuntimeError(f"{who}: input_lengths must be an int tensor, got {lx.dtype}")
        if int(lx.min()) < 0 or int(lx.max()) > T:
            raise RuntimeError(f"{who}: the chunk's frame lengths must lie in [0, Tc={T}], got min {int(lx.min())}, max {int(lx.max())}")
    if reset is not None:
        if reset.dim() != 1 or reset.numel() != N or reset.dtype.is_floating_point:
            raise RuntimeError(f"{who}: reset must be a bool or int tensor of shape ({N},), got {reset.dtype} of shape {tuple(reset.shape)}")
    _check_beam_lm_args(lm, alpha, beta, return_lm_scores, V)
    W, K, C, cap = int(beam_size), int(nbest), int(top_classes), int(max_hyp_len)
    if state is not None:
        if not isinstance(state, BeamState):
            raise RuntimeError(f"{who}: state must be a BeamState (what this call returns) or None, got {type(state).__name__}")
        mine = dict(beam_size=W, top_classes=C, blank=int(blank), max_hyp_len=cap, alpha=float(alpha), beta=float(beta))
        for k in BeamState.FIELDS:
            if (getattr(state, k) is not lm) if k == "lm" else (getattr(state, k) != mine[k]):
                raise RuntimeError(f"{who}: the state was made with {k}={getattr(state, k)!r}, this call has {k}={(lm if k == 'lm' else mine[k])!r}: "
                                   f"a state continues only under the values it was made with")
        if len(state) != N:
            raise RuntimeError(f"{who}: the state holds {len(state)} utterances, the chunk {N}")
    if not log_probs.is_cuda:                  # (after the checks of the arguments: those need no device)
        raise RuntimeError(f"{who}: log_probs must be on the GPU (there is no CPU path)")
    assert log_probs.is_contiguous()
    dev = log_probs.device
    if lx.is_cuda and lx.device != dev:
        raise RuntimeError(f"{who}: input_lengths is on {lx.device}, log_probs on {dev}")
    rec = _lib.crf_ctc_beam_state_record_bytes(W, cap)
    if rec < 0:
        _check(1)
    if state is not None and (state.records.device != dev or tuple(state.records.shape) != (N, rec) or state.records.dtype != torch.uint8):
        raise RuntimeError(f"{who}: the state's records are {tuple(state.records.shape)} {state.records.dtype} on {state.records.device}, "
                           f"expect ({N}, {rec}) uint8 on {dev}")
    lx_d = lx.contiguous() if lx.is_cuda else _h2d_async(lx.to(torch.int32).reshape(-1), dev)
    reset_d = None
    if reset is not None:
        reset_d = (reset.to(dev) != 0).to(torch.int32) if reset.is_cuda else _h2d_async((reset != 0).to(torch.int32), dev)
    rec_in = state.records.contiguous() if state is not None else None
    H = N * K
    ws_bytes = _lib.crf_ctc_beam_chunk_workspace_bytes(N, T, V, W, C)
    ws = _new_ws(ws_bytes, dev)
    rec_out = torch.empty((N, rec), dtype=torch.uint8, device=dev)
    hyps = torch.empty((H, cap), dtype=torch.int32, device=dev)
    hyp_len = torch.empty(H, dtype=torch.int32, device=dev)
    scores = torch.empty(H, dtype=torch.float32, device=dev)
    trace = torch.empty((N, T, W), dtype=torch.int32, device=dev) if return_trace else None
    lm_scores = torch.empty(H, dtype=torch.float32, device=dev) if return_lm_scores else None
    tables = None
    if lm is not None:
        tables, _keep = lm.tables(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = _lib.crf_ctc_beam_chunk(_ptr(log_probs), _FUSED_DTYPES[log_probs.dtype], 1 if time_major else 0, int(blank), 1 if fused else 0,
                                     _ptr(lx_d), N, T, V, W, K, C, ctypes.byref(tables) if tables is not None else _vp(0), float(alpha),
                                     float(beta), _ptr(rec_in), _ptr(reset_d), _ptr(rec_out), cap, _ptr(hyps), _ptr(hyp_len), _ptr(scores),
                                     _ptr(lm_scores), _ptr(trace), _ptr(ws), ws_bytes, _vp(stream))
    _check(rc)
    del lx_d, reset_d
    return BeamState(rec_out, W, C, int(blank), cap, lm, alpha, beta), hyps, hyp_len, scores, trace, lm_scores


EDIT_MAX_REF_LEN = 2047      # longest reference crf_ctc_edit_distance takes (kMaxCtcLabelLen; include/ctc_crf_hip.h)
EDIT_STRIP_ROWS = 512        # references beyond this many tokens are walked in strips, which hold hypothesis rows of up to ...
EDIT_STRIP_MAX_COLS = 8192   # ... this many entries


def _check_edit_args(hyps: torch.Tensor, hyp_lengths: torch.Tensor, labels: torch.Tensor, label_lengths: torch.Tensor,
                     hyp_utt: Optional[torch.Tensor]):
    """The host checks of ctc_edit_distance, each with the offending value in the message; none needs a device.
    -> (H, W, N, ly32, lab32, max_ref_len)."""
    who = "ctc_edit_distance"
    if hyps.dim() != 2:
        raise RuntimeError(f"{who}: expect hyps of shape (H, W), got {hyps.dim()} dimensions")
    H, W = hyps.shape
    if hyps.dtype != torch.int32:
        raise RuntimeError(f"{who}: expect int32 hyps, got {hyps.dtype}")
    if hyp_lengths.dtype != torch.int32:
        raise RuntimeError(f"{who}: expect int32 hyp_lengths, got {hyp_lengths.dtype}")
    if hyp_lengths.dim() != 1 or hyp_lengths.numel() != H:
        raise RuntimeError(f"{who}: expect hyp_lengths of shape ({H},), one per row of hyps, got {tuple(hyp_lengths.shape)}")
    if labels.is_cuda or label_lengths.is_cuda:
        raise RuntimeError(f"{who}: labels and label_lengths are CPU tensors")
    if labels.is_floating_point() or label_lengths.is_floating_point():
        raise RuntimeError(f"{who}: expect integer labels and label_lengths, got {labels.dtype} and {label_lengths.dtype}")
    if label_lengths.dim() != 1:
        raise RuntimeError(f"{who}: expect label_lengths of shape (N,), got {label_lengths.dim()} dimensions")
    ly32 = label_lengths.to(torch.int32)
    lab32 = labels.to(torch.int32).reshape(-1)
    N = ly32.numel()
    if N == 0:
        raise RuntimeError(f"{who}: no utterances")
    if int(ly32.min()) < 0:
        raise RuntimeError("negative label length")
    if int(ly32.sum()) > lab32.numel():
        raise RuntimeError(f"sum(label_lengths)={int(ly32.sum())} exceeds len(labels)={lab32.numel()}")
    max_ref = int(ly32.max())
    if max_ref > EDIT_MAX_REF_LEN:
        raise RuntimeError(f"{who}: label length {max_ref} > {EDIT_MAX_REF_LEN} not supported by this build")
    if max_ref > EDIT_STRIP_ROWS and W > EDIT_STRIP_MAX_COLS:
        raise RuntimeError(f"{who}: rows of hyps of {W} > {EDIT_STRIP_MAX_COLS} entries with references of more than {EDIT_STRIP_ROWS} "
                           f"tokens not supported by this build")
    if hyp_utt is None:
        if H != N:
            raise RuntimeError(f"{who}: hyp_utt=None takes hypothesis h against utterance h: expect {N} hypotheses, got {H}")
    else:
        if hyp_utt.dtype != torch.int32:
            raise RuntimeError(f"{who}: expect int32 hyp_utt, got {hyp_utt.dtype}")
        if hyp_utt.dim() != 1 or hyp_utt.numel() != H:
            raise RuntimeError(f"{who}: expect hyp_utt of shape ({H},), one per row of hyps, got {tuple(hyp_utt.shape)}")
    if H * max(W, 1) > 2 ** 31 - 1:
        raise RuntimeError(f"{who}: H * W = {H * W} > INT32_MAX")
    return H, W, N, ly32, lab32, max_ref


def ctc_edit_distance(hyps: torch.Tensor, hyp_lengths: torch.Tensor, labels: torch.Tensor, label_lengths: torch.Tensor,
                      hyp_utt: Optional[torch.Tensor] = None, return_ops: bool = False):
    """Token edit distance of H hypotheses to their utterances' transcripts (include/ctc_crf_hip.h ``crf_ctc_edit_distance``).

    hyps [H,W] int32, hyp_lengths [H] int32 and hyp_utt [H] int32 (None: H = N, hypothesis h against utterance h) on the GPU, as ctc_sample
    / ctc_greedy / ctc_beam_search return them; labels flat and label_lengths [N] int tensors on the CPU, staged in one copy.  Returns
    (dist [H] int32, ops [H,3] int32 = (nsub, ndel, nins) or None) on the device, no host synchronisation; a row whose hyp_utt or hyp_lengths
    entry is out of range takes -1."""
    who = "ctc_edit_distance"
    H, W, N, ly32, lab32, max_ref = _check_edit_args(hyps, hyp_lengths, labels, label_lengths, hyp_utt)
    if not hyps.is_cuda:                       # (after the checks of the arguments: those need no device)
        raise RuntimeError(f"{who}: hyps must be on the GPU (there is no CPU path)")
    dev = hyps.device
    if hyp_lengths.device != dev or (hyp_utt is not None and hyp_utt.device != dev):
        raise RuntimeError(f"{who}: hyp_lengths and hyp_utt must be on the device of hyps ({dev})")
    dist = torch.empty(H, dtype=torch.int32, device=dev)
    ops = torch.empty((H, 3), dtype=torch.int32, device=dev) if return_ops else None
    if H == 0:
        return dist, ops
    hyps = hyps.contiguous() if W > 0 else torch.zeros((H, 1), dtype=torch.int32, device=dev)   # (no row of width 0 in the C ABI)
    hyp_lengths = hyp_lengths.contiguous()
    nlab = int(ly32.sum())
    off = (torch.cumsum(ly32, 0, dtype=torch.int32) - ly32).to(torch.int32)
    meta = _h2d_async(torch.cat([ly32, off, lab32[:nlab] if nlab else torch.zeros(1, dtype=torch.int32)]), dev)
    len_d, off_d, lab_d = meta[:N], meta[N:2 * N], meta[2 * N:]
    utt_d = torch.arange(N, dtype=torch.int32, device=dev) if hyp_utt is None else hyp_utt.contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = _lib.crf_ctc_edit_distance(_ptr(hyps), max(W, 1), _ptr(hyp_lengths), _ptr(utt_d), _ptr(lab_d), _ptr(off_d), _ptr(len_d), N, H,
                                        max_ref, _ptr(dist), _ptr(ops), _vp(stream))
    _check(rc)
    del meta
    return dist, ops


NGRAM_SCORE_MAX_WIDTH = 8192   # widest row crf_ngram_score takes (kNgramMaxStride; include/ctc_crf_hip.h)


def _check_ngram_score_args(hyps: torch.Tensor, hyp_lengths: torch.Tensor, lm, eos: bool):
    """The host checks of ngram_score, each with the offending value in the message; none needs a device.  -> (H, W)."""
    from ..ngram_lm import NgramLM
    who = "ngram_score"
    if not isinstance(lm, NgramLM):
        raise RuntimeError(f"{who}: lm must be an NgramLM (cat_amd.ngram_lm), got {type(lm).__name__}: {lm!r}")
    if hyps.dim() != 2 or hyps.dtype != torch.int32:
        raise RuntimeError(f"{who}: expect hyps as padded rows (H, W) of int32, got {tuple(hyps.shape)} of {hyps.dtype}")
    H, W = hyps.shape
    if hyp_lengths.dtype != torch.int32 or hyp_lengths.dim() != 1 or hyp_lengths.numel() != H:
        raise RuntimeError(f"{who}: expect hyp_lengths as an int32 tensor ({H},), one entry per row of hyps, got {tuple(hyp_lengths.shape)} "
                           f"of {hyp_lengths.dtype}")
    if W > NGRAM_SCORE_MAX_WIDTH:
        raise RuntimeError(f"{who}: rows of hyps of {W} > {NGRAM_SCORE_MAX_WIDTH} entries not supported by this build")
    if eos and lm.eos_logp is None:
        raise ValueError(f"{who}: eos=True needs a model with a </s> unigram (lm.eos_logp is None)")
    if not hyps.is_cuda or not hyp_lengths.is_cuda:
        raise ValueError(f"{who}: hyps and hyp_lengths must be on the GPU; on the host NgramLM.score(tokens, eos) and NgramLM.token_scores "
                         f"give the same values")
    if hyp_lengths.device != hyps.device:
        raise RuntimeError(f"{who}: hyp_lengths lies on {hyp_lengths.device}, hyps on {hyps.device}")
    return H, W


def ngram_score(hyps: torch.Tensor, hyp_lengths: torch.Tensor, lm, bos: bool = True, eos: bool = False, return_token_scores: bool = False):
    """n-gram LM scores of hypothesis rows on the GPU (include/ctc_crf_hip.h ``crf_ngram_score``): per row log P_lm in natural log.

    hyps [H,W] int32 and hyp_lengths [H] int32 on one GPU, as ctc_sample / ctc_greedy / ctc_beam_search return them (rows a stride apart are
    taken as ctc_score takes them); lm an NgramLM (tables and eos_logp are uploaded once per device and kept).  bos: the walk starts in
    lm.start, else at the root; eos: plus lm.eos_logp[state behind the last token].  Returns (scores [H] f32, invalid [H] int32) and, with
    return_token_scores, (token_logp [H,W] f32, token_order [H,W] int32: per position the value of NgramLM.lookup and the length of the
    n-gram found, 0 behind the length) -- on the device, without autograd history and without a host synchronisation.  A row whose length
    lies outside [0, W] or that holds a token outside [0, lm.vocab_size) among its first hyp_lengths[h] scores -inf with invalid = 1.  A row's
    outputs are the same bits in any batch.

    Rescoring an N-best list (ac = ctc_score's or the search's scores, rows of one utterance adjacent)::

        lm_s, _ = ngram_score(hyps, hyp_lengths, lm, eos=True)
        total = ac + alpha * lm_s + beta * hyp_lengths
        best = total.view(N, nbest).argmax(1)

    The weight grid of lmweight_search.py, with dist = ctc_edit_distance(...)[0] and alphas, betas of shape (G,)::

        total = ac + alphas[:, None] * lm_s + betas[:, None] * hyp_lengths            # (G, H)
        best = total.view(G, N, nbest).argmax(2)                                      # (G, N)
        errs = dist.view(N, nbest).expand(G, N, nbest).gather(2, best[..., None]).sum((1, 2))
    """
    H, W = _check_ngram_score_args(hyps, hyp_lengths, lm, eos)
    dev = hyps.device
    stride = max(W, 1)
    scores = torch.empty(H, dtype=torch.float32, device=dev)
    invalid = torch.empty(H, dtype=torch.int32, device=dev)
    tok_lp = torch.empty((H, stride), dtype=torch.float32, device=dev) if return_token_scores else None
    tok_or = torch.empty((H, stride), dtype=torch.int32, device=dev) if return_token_scores else None
    if H > 0:
        # (the C ABI has one stride for the rows and the per-token outputs, and a length up to it is valid: rows further apart are copied)
        # (no row of width 0 in the C ABI: one word that is no token, so that only length 0 is valid)
        rows = hyps.detach().contiguous() if W > 0 else torch.full((H, 1), -1, dtype=torch.int32, device=dev)
        tables, keep = lm.tables(dev)
        eos_t = keep.get("eos_logp") if eos else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            rc = _lib.crf_ngram_score(ctypes.byref(tables), _ptr(eos_t), _ptr(rows), stride, _ptr(hyp_lengths.contiguous()), H, 1 if bos else 0,
                                      1 if eos else 0, _ptr(scores), _ptr(invalid), _ptr(tok_lp), _ptr(tok_or), _vp(stream))
        _check(rc)
    if return_token_scores:
        return scores, invalid, tok_lp[:, :W], tok_or[:, :W]
    return scores, invalid


RNNT_MAX_LABELS = 1023       # longest label sequence crf_rnnt_loss takes (one thread per lattice column; include/ctc_crf_hip.h)
RNNT_MAX_VOCAB = 8192


class RnntCall:
    """What rnnt_loss_fwd leaves for rnnt_loss_bwd: the C call's arguments (the staged tensors are kept alive here) and the workspace."""

    def __init__(self, x, fused, blank, labels, lx, ly, N, T, U1, V, rows, nlab, ws):
        self.x, self.fused, self.blank, self.labels, self.lx, self.ly = x, fused, blank, labels, lx, ly
        self.N, self.T, self.U1, self.V, self.rows, self.nlab, self.ws = N, T, U1, V, rows, nlab, ws


def _check_rnnt_args(x: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int, compact: bool, fused: bool):
    """The host checks of rnnt_loss, each with the offending value in the message; none needs a device.  -> (N, T, U1, V, rows, nlab) with
    rows = nlab = -1 in the padded layout; T and U1 are bounds on the lengths in the compact one."""
    who = "rnnt_loss"
    if fused:
        if x.dtype not in _FUSED_DTYPES:
            raise RuntimeError(f"{who}: fuse_log_softmax expects float32, bfloat16 or float16 joiner output, got {x.dtype}")
    elif x.dtype != torch.float32:
        raise RuntimeError(f"{who}: expect normalised float32 log_probs (or fuse_log_softmax=True for raw output), got {x.dtype}")
    if labels.dtype != torch.int32 or lx.dtype != torch.int32 or ly.dtype != torch.int32:
        raise RuntimeError(f"{who}: labels, frames_lengths and labels_lengths must be int32, got {labels.dtype}, {lx.dtype}, {ly.dtype}")
    if lx.dim() != 1 or ly.dim() != 1 or lx.numel() != ly.numel() or lx.numel() == 0:
        raise RuntimeError(f"{who}: expect frames_lengths and labels_lengths as (N,) with N >= 1, got {tuple(lx.shape)} and {tuple(ly.shape)}")
    N = lx.numel()
    V = x.shape[-1]
    if not 1 <= V <= RNNT_MAX_VOCAB:
        raise RuntimeError(f"{who}: V = {V} outside [1, {RNNT_MAX_VOCAB}] not supported by this build")
    if not 0 <= blank < V:
        raise RuntimeError(f"{who}: blank must lie in [0, V-1={V - 1}], got {blank}")
    host = not lx.is_cuda and not ly.is_cuda
    if lx.is_cuda != ly.is_cuda:
        raise RuntimeError(f"{who}: frames_lengths and labels_lengths must both be on the CPU or both on the GPU")
    if compact:
        if x.dim() != 2 or labels.dim() != 1:
            raise RuntimeError(f"{who}: compact expects log_probs (sum T_n (U_n + 1), V) and labels (sum U_n,), got {tuple(x.shape)} and {tuple(labels.shape)}")
        rows, nlab = x.shape[0], labels.numel()
        if rows < 1:
            raise RuntimeError(f"{who}: no rows")
        T, U1 = rows, min(nlab, RNNT_MAX_LABELS) + 1
        if host:
            if int(lx.min()) < 1 or int(ly.min()) < 0:
                raise ValueError(f"{who}: frames_lengths must be >= 1 and labels_lengths >= 0, got minima {int(lx.min())} and {int(ly.min())}")
            if int(ly.max()) > RNNT_MAX_LABELS:
                raise ValueError(f"{who}: labels_lengths up to {int(ly.max())} > {RNNT_MAX_LABELS} not supported by this build")
            want = int((lx.long() * (ly.long() + 1)).sum())
            if want != rows or int(ly.sum()) != nlab:
                raise ValueError(f"{who}: the lengths give {want} rows and {int(ly.sum())} labels, log_probs has {rows} and labels {nlab}")
            T, U1 = int(lx.max()), int(ly.max()) + 1
        return N, T, U1, V, rows, nlab
    if x.dim() != 4 or x.shape[0] != N:
        raise RuntimeError(f"{who}: expect log_probs (N={N}, T, U+1, V), got {tuple(x.shape)}")
    _, T, U1, _ = x.shape
    if T < 1 or U1 < 1:
        raise RuntimeError(f"{who}: empty lattice {tuple(x.shape)}")
    if U1 - 1 > RNNT_MAX_LABELS:
        raise RuntimeError(f"{who}: U = {U1 - 1} > {RNNT_MAX_LABELS} not supported by this build")
    if tuple(labels.shape) != (N, U1 - 1):
        raise RuntimeError(f"{who}: expect labels (N={N}, U={U1 - 1}), got {tuple(labels.shape)}")
    if host:
        if int(lx.min()) < 1 or int(lx.max()) > T:
            raise ValueError(f"{who}: frames_lengths must lie in [1, T={T}], got [{int(lx.min())}, {int(lx.max())}]")
        if int(ly.min()) < 0 or int(ly.max()) > U1 - 1:
            raise ValueError(f"{who}: labels_lengths must lie in [0, U={U1 - 1}], got [{int(ly.min())}, {int(ly.max())}]")
    return N, T, U1, V, -1, -1


def rnnt_loss_fwd(x: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int = 0, compact: bool = False,
                  fused: bool = False):
    """The forward of the RNN-T loss (include/ctc_crf_hip.h ``crf_rnnt_loss`` / ``crf_rnnt_loss_logits``) -> (costs [N] f32, invalid [N]
    int32, RnntCall for rnnt_loss_bwd) on the device, without a host synchronisation when the lengths are on the device."""
    N, T, U1, V, rows, nlab = _check_rnnt_args(x, labels, lx, ly, blank, compact, fused)
    if not x.is_cuda:
        raise RuntimeError("rnnt_loss: log_probs must be on the GPU (there is no CPU path)")
    dev = x.device
    x = x.detach().contiguous()
    lab_d = labels.to(dev).contiguous() if labels.numel() else torch.zeros(1, dtype=torch.int32, device=dev)   # (no NULL in the C ABI)
    if lx.is_cuda:
        lx_d, ly_d = lx.contiguous(), ly.contiguous()
    else:
        meta = _h2d_async(torch.cat([lx, ly]), dev)
        lx_d, ly_d = meta[:N], meta[N:]
    costs = torch.empty(N, dtype=torch.float32, device=dev)
    invalid = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _new_ws(_lib.crf_rnnt_workspace_bytes(N, T, U1, V, rows), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tail = (blank, _ptr(lab_d), _ptr(lx_d), _ptr(ly_d), N, T, U1, V, rows, nlab, _ptr(costs), _ptr(invalid), _ptr(ws), ws.numel(), _vp(stream))
    with torch.cuda.device(dev):
        rc = _lib.crf_rnnt_loss_logits(_ptr(x), _FUSED_DTYPES[x.dtype], *tail) if fused else _lib.crf_rnnt_loss(_ptr(x), *tail)
    _check(rc)
    return costs, invalid, RnntCall(x, fused, blank, lab_d, lx_d, ly_d, N, T, U1, V, rows, nlab, ws)


def rnnt_loss_bwd(call: RnntCall, grad_output: torch.Tensor, grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward on the forward's workspace (``crf_rnnt_grad`` / ``crf_rnnt_grad_logits``): grad_output [N] is d loss / d costs; returns
    the gradient in the input's shape and dtype, every element written by the kernel (grad_out: a contiguous tensor of that shape and
    dtype to write into, whatever it holds)."""
    c = call
    dev = c.x.device
    w = grad_output.detach().to(device=dev, dtype=torch.float32).contiguous()
    if w.numel() != c.N:
        raise RuntimeError(f"rnnt_loss: expect grad_output ({c.N},), got {tuple(grad_output.shape)}")
    grad = torch.empty_like(c.x) if grad_out is None else grad_out
    if grad.shape != c.x.shape or grad.dtype != c.x.dtype or grad.device != dev or not grad.is_contiguous():
        raise RuntimeError("rnnt_loss: grad_out must be contiguous, of the input's shape and dtype and on its device")
    stream = torch.cuda.current_stream(dev).cuda_stream
    tail = (c.blank, _ptr(c.labels), _ptr(c.lx), _ptr(c.ly), c.N, c.T, c.U1, c.V, c.rows, c.nlab, _ptr(w), _ptr(grad), _ptr(c.ws), c.ws.numel(),
            _vp(stream))
    with torch.cuda.device(dev):
        rc = _lib.crf_rnnt_grad_logits(_ptr(c.x), _FUSED_DTYPES[c.x.dtype], *tail) if c.fused else _lib.crf_rnnt_grad(_ptr(c.x), *tail)
    _check(rc)
    return grad


class CtctCall:
    """What ctct_loss_fwd leaves for ctct_loss_bwd: the C call's arguments (the staged tensors are kept alive here) and the workspace."""

    def __init__(self, x, fused, blank, labels, lx, ly, N, T, U1, V, ws):
        self.x, self.fused, self.blank, self.labels, self.lx, self.ly = x, fused, blank, labels, lx, ly
        self.N, self.T, self.U1, self.V, self.ws = N, T, U1, V, ws


def _check_ctct_args(x: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int, fused: bool):
    """The host checks of ctct_loss, each a ValueError with the offending value in the message; none needs a device.  -> (N, T, U1, V)."""
    who = "ctct_loss"
    if fused:
        if x.dtype not in _FUSED_DTYPES:
            raise ValueError(f"{who}: fuse_log_softmax expects float32, bfloat16 or float16 joiner output, got {x.dtype}")
    elif x.dtype != torch.float32:
        raise ValueError(f"{who}: expect normalised float32 log_probs (or fuse_log_softmax=True for raw output), got {x.dtype}")
    if labels.dtype != torch.int32 or lx.dtype != torch.int32 or ly.dtype != torch.int32:
        raise ValueError(f"{who}: labels, frames_lengths and labels_lengths must be int32, got {labels.dtype}, {lx.dtype}, {ly.dtype}")
    if lx.dim() != 1 or ly.dim() != 1 or lx.numel() != ly.numel() or lx.numel() == 0:
        raise ValueError(f"{who}: expect frames_lengths and labels_lengths as (N,) with N >= 1, got {tuple(lx.shape)} and {tuple(ly.shape)}")
    N = lx.numel()
    if x.dim() != 4 or x.shape[0] != N:
        raise ValueError(f"{who}: expect log_probs (N={N}, T, U+1, V), got {tuple(x.shape)}")
    _, T, U1, V = x.shape
    if T < 1 or U1 < 1:
        raise ValueError(f"{who}: empty lattice {tuple(x.shape)}")
    if not 1 <= V <= RNNT_MAX_VOCAB:
        raise ValueError(f"{who}: V = {V} outside [1, {RNNT_MAX_VOCAB}] not supported by this build")
    if not 0 <= blank < V:
        raise ValueError(f"{who}: blank must lie in [0, V-1={V - 1}], got {blank}")
    if U1 - 1 > RNNT_MAX_LABELS:
        raise ValueError(f"{who}: U = {U1 - 1} > {RNNT_MAX_LABELS} not supported by this build")
    if tuple(labels.shape) != (N, U1 - 1):
        raise ValueError(f"{who}: expect labels (N={N}, U={U1 - 1}), got {tuple(labels.shape)}")
    if not x.is_contiguous() or not labels.is_contiguous():
        raise ValueError(f"{who}: log_probs and labels must be contiguous (the joiner output is read in place)")
    if lx.is_cuda != ly.is_cuda:
        raise ValueError(f"{who}: frames_lengths and labels_lengths must both be on the CPU or both on the GPU")
    if not lx.is_cuda:
        if int(lx.min()) < 1 or int(lx.max()) > T:
            raise ValueError(f"{who}: frames_lengths must lie in [1, T={T}], got [{int(lx.min())}, {int(lx.max())}]")
        if int(ly.min()) < 0 or int(ly.max()) > U1 - 1:
            raise ValueError(f"{who}: labels_lengths must lie in [0, U={U1 - 1}], got [{int(ly.min())}, {int(ly.max())}]")
    return N, T, U1, V


def ctct_loss_fwd(x: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int = 0, fused: bool = False):
    """The forward of the CTC-Transducer loss (include/ctc_crf_hip.h ``crf_ctct_loss`` / ``crf_ctct_loss_logits``) -> (costs [N] f32, invalid
    [N] int32, CtctCall for ctct_loss_bwd) on the device, without a host synchronisation when the lengths are on the device."""
    N, T, U1, V = _check_ctct_args(x, labels, lx, ly, blank, fused)
    if not x.is_cuda:
        raise RuntimeError("ctct_loss: log_probs must be on the GPU (there is no CPU path)")
    dev = x.device
    x = x.detach()
    lab_d = labels.to(dev) if labels.numel() else torch.zeros(1, dtype=torch.int32, device=dev)   # (no NULL in the C ABI)
    if lx.is_cuda:
        lx_d, ly_d = lx.contiguous(), ly.contiguous()
    else:
        meta = _h2d_async(torch.cat([lx, ly]), dev)
        lx_d, ly_d = meta[:N], meta[N:]
    costs = torch.empty(N, dtype=torch.float32, device=dev)
    invalid = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _new_ws(_lib.crf_ctct_workspace_bytes(N, T, U1, V), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tail = (blank, _ptr(lab_d), _ptr(lx_d), _ptr(ly_d), N, T, U1, V, _ptr(costs), _ptr(invalid), _ptr(ws), ws.numel(), _vp(stream))
    with torch.cuda.device(dev):
        rc = _lib.crf_ctct_loss_logits(_ptr(x), _FUSED_DTYPES[x.dtype], *tail) if fused else _lib.crf_ctct_loss(_ptr(x), *tail)
    _check(rc)
    return costs, invalid, CtctCall(x, fused, blank, lab_d, lx_d, ly_d, N, T, U1, V, ws)


def ctct_loss_bwd(call: CtctCall, grad_output: torch.Tensor, grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward on the forward's workspace (``crf_ctct_grad`` / ``crf_ctct_grad_logits``): grad_output [N] is d loss / d costs; returns
    the gradient in the input's shape and dtype, every element written by the kernel (grad_out: a contiguous tensor of that shape and
    dtype to write into, whatever it holds)."""
    c = call
    dev = c.x.device
    w = grad_output.detach().to(device=dev, dtype=torch.float32).contiguous()
    if w.numel() != c.N:
        raise RuntimeError(f"ctct_loss: expect grad_output ({c.N},), got {tuple(grad_output.shape)}")
    grad = torch.empty_like(c.x) if grad_out is None else grad_out
    if grad.shape != c.x.shape or grad.dtype != c.x.dtype or grad.device != dev or not grad.is_contiguous():
        raise RuntimeError("ctct_loss: grad_out must be contiguous, of the input's shape and dtype and on its device")
    stream = torch.cuda.current_stream(dev).cuda_stream
    tail = (c.blank, _ptr(c.labels), _ptr(c.lx), _ptr(c.ly), c.N, c.T, c.U1, c.V, _ptr(w), _ptr(grad), _ptr(c.ws), c.ws.numel(), _vp(stream))
    with torch.cuda.device(dev):
        rc = _lib.crf_ctct_grad_logits(_ptr(c.x), _FUSED_DTYPES[c.x.dtype], *tail) if c.fused else _lib.crf_ctct_grad(_ptr(c.x), *tail)
    _check(rc)
    return grad


class RnntSimpleCall:
    """What rnnt_simple_fwd leaves for rnnt_simple_bwd: the C call's arguments (the staged tensors are kept alive here) and the workspace."""

    def __init__(self, f, g, blank, labels, lx, ly, N, T, U1, V, ws):
        self.f, self.g, self.blank, self.labels, self.lx, self.ly = f, g, blank, labels, lx, ly
        self.N, self.T, self.U1, self.V, self.ws = N, T, U1, V, ws


def _check_rnnt_simple_args(f: torch.Tensor, g: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int):
    """The host checks of rnnt_loss_simple, each with the offending value in the message; none needs a device.  -> (N, T, U1, V)."""
    who = "rnnt_loss_simple"
    if f.dtype != g.dtype or f.dtype not in _FUSED_DTYPES:
        raise ValueError(f"{who}: f_enc and g_pred must be of one dtype among float32, bfloat16 and float16, got {f.dtype} and {g.dtype}")
    if f.dim() != 3 or g.dim() != 3:
        raise ValueError(f"{who}: expect f_enc (N, T, V) and g_pred (N, U+1, V), got {tuple(f.shape)} and {tuple(g.shape)}")
    if f.shape[0] != g.shape[0]:
        raise ValueError(f"{who}: f_enc has {f.shape[0]} utterances, g_pred {g.shape[0]}")
    if f.shape[2] != g.shape[2]:
        raise ValueError(f"{who}: f_enc has {f.shape[2]} classes, g_pred {g.shape[2]}")
    if not f.is_contiguous() or not g.is_contiguous():
        raise ValueError(f"{who}: f_enc and g_pred must be contiguous (they are read in place)")
    N, T, V = f.shape
    U1 = g.shape[1]
    if labels.dtype != torch.int32 or lx.dtype != torch.int32 or ly.dtype != torch.int32:
        raise RuntimeError(f"{who}: labels, frames_lengths and labels_lengths must be int32, got {labels.dtype}, {lx.dtype}, {ly.dtype}")
    if lx.dim() != 1 or ly.dim() != 1 or lx.numel() != N or ly.numel() != N or N == 0:
        raise ValueError(f"{who}: expect frames_lengths and labels_lengths as (N={N},) with N >= 1, got {tuple(lx.shape)} and {tuple(ly.shape)}")
    if T < 1 or U1 < 1:
        raise ValueError(f"{who}: empty lattice: f_enc {tuple(f.shape)}, g_pred {tuple(g.shape)}")
    if not 1 <= V <= RNNT_MAX_VOCAB:
        raise ValueError(f"{who}: V = {V} outside [1, {RNNT_MAX_VOCAB}] not supported by this build")
    if U1 - 1 > RNNT_MAX_LABELS:
        raise ValueError(f"{who}: U = {U1 - 1} > {RNNT_MAX_LABELS} not supported by this build")
    if not 0 <= blank < V:
        raise ValueError(f"{who}: blank must lie in [0, V-1={V - 1}], got {blank}")
    if tuple(labels.shape) != (N, U1 - 1):
        raise ValueError(f"{who}: expect labels (N={N}, U={U1 - 1}), got {tuple(labels.shape)}")
    if lx.is_cuda != ly.is_cuda:
        raise RuntimeError(f"{who}: frames_lengths and labels_lengths must both be on the CPU or both on the GPU")
    if not lx.is_cuda:
        if int(lx.min()) < 1 or int(lx.max()) > T:
            raise ValueError(f"{who}: frames_lengths must lie in [1, T={T}], got [{int(lx.min())}, {int(lx.max())}]")
        if int(ly.min()) < 0 or int(ly.max()) > U1 - 1:
            raise ValueError(f"{who}: labels_lengths must lie in [0, U={U1 - 1}], got [{int(ly.min())}, {int(ly.max())}]")
    return N, T, U1, V


def rnnt_simple_fwd(f: torch.Tensor, g: torch.Tensor, labels: torch.Tensor, lx: torch.Tensor, ly: torch.Tensor, blank: int = 0):
    """The forward of the RNN-T loss of the joiner f + g (include/ctc_crf_hip.h ``crf_rnnt_simple_loss``) -> (costs [N] f32, invalid [N]
    int32, RnntSimpleCall for rnnt_simple_bwd) on the device, without a host synchronisation when the lengths are on the device.  f and g
    are read in place: nothing of size T (U + 1) V is allocated."""
    N, T, U1, V = _check_rnnt_simple_args(f, g, labels, lx, ly, blank)
    if not f.is_cuda or g.device != f.device:
        raise RuntimeError("rnnt_loss_simple: f_enc and g_pred must be on one GPU (there is no CPU path)")
    dev = f.device
    f, g = f.detach(), g.detach()
    lab_d = labels.to(dev).contiguous() if labels.numel() else torch.zeros(1, dtype=torch.int32, device=dev)   # (no NULL in the C ABI)
    if lx.is_cuda:
        lx_d, ly_d = lx.contiguous(), ly.contiguous()
    else:
        meta = _h2d_async(torch.cat([lx, ly]), dev)
        lx_d, ly_d = meta[:N], meta[N:]
    costs = torch.empty(N, dtype=torch.float32, device=dev)
    invalid = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _new_ws(_lib.crf_rnnt_simple_workspace_bytes(N, T, U1, V), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = _lib.crf_rnnt_simple_loss(_ptr(f), _ptr(g), _FUSED_DTYPES[f.dtype], blank, _ptr(lab_d), _ptr(lx_d), _ptr(ly_d), N, T, U1, V,
                                       _ptr(costs), _ptr(invalid), _ptr(ws), ws.numel(), _vp(stream))
    _check(rc)
    return costs, invalid, RnntSimpleCall(f, g, blank, lab_d, lx_d, ly_d, N, T, U1, V, ws)


def rnnt_simple_bwd(call: RnntSimpleCall, grad_output: torch.Tensor, want_f: bool = True, want_g: bool = True,
                    grad_out: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None):
    """The backward on the forward's workspace (``crf_rnnt_simple_grad``): grad_output [N] is d loss / d costs; returns (grad_f, grad_g) in
    the inputs' shapes and dtype, every element written by the kernels, None where want_f / want_g is false (that gradient is not formed).
    grad_out: a pair of contiguous tensors of those shapes and that dtype to write into, whatever they hold."""
    c = call
    dev = c.f.device
    w = grad_output.detach().to(device=dev, dtype=torch.float32).contiguous()
    if w.numel() != c.N:
        raise RuntimeError(f"rnnt_loss_simple: expect grad_output ({c.N},), got {tuple(grad_output.shape)}")
    outs = []
    for k, (want, like) in enumerate(((want_f, c.f), (want_g, c.g))):
        t = None
        if want:
            t = grad_out[k] if grad_out is not None and grad_out[k] is not None else torch.empty_like(like)
            if t.shape != like.shape or t.dtype != like.dtype or t.device != dev or not t.is_contiguous():
                raise RuntimeError("rnnt_loss_simple: grad_out must be contiguous, of the inputs' shapes and dtype and on their device")
        outs.append(t)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = _lib.crf_rnnt_simple_grad(_ptr(c.f), _ptr(c.g), _FUSED_DTYPES[c.f.dtype], c.blank, _ptr(c.labels), _ptr(c.lx), _ptr(c.ly), c.N, c.T,
                                       c.U1, c.V, _ptr(w), _ptr(outs[0]), _ptr(outs[1]), _ptr(c.ws), c.ws.numel(), _vp(stream))
    _check(rc)
    return outs[0], outs[1]


def gpu_den(logits: torch.Tensor, grad_net: torch.Tensor, input_lengths: torch.Tensor,
            costs_alpha: torch.Tensor, costs_beta: torch.Tensor) -> None:
    """Same signature and in-place outputs as the reference's ``_C.gpu_den`` (binding.cpp:65-84)."""
    _, g, ex = loss_fwd_bwd(logits.contiguous(), None, input_lengths, None, 1.0, 0.0, graph_for(logits.device), True)
    grad_net.copy_(g)
    costs_alpha.copy_(ex["costs_alpha"])
    costs_beta.copy_(ex["costs_beta"])


def gpu_ctc(probs: torch.Tensor, grads: torch.Tensor, labels: torch.Tensor, label_sizes: torch.Tensor,
            sizes: torch.Tensor, minibatch_size: int, costs: torch.Tensor, blank_label: int = 0) -> None:
    """Same signature as the reference's ``_C.gpu_ctc`` (binding.cpp:86-117): probs/grads are
    [T,N,V] (the reference's time-major layout, __init__.py:70), any blank_label in [0, V), costs is a
    CPU tensor receiving +loglike.  The kernels read probs and write grads in that layout in place
    (crf_ctc_fwd_bwd, time_major = 1): no transposed copies."""
    assert probs.size(1) == minibatch_size
    direct = (grads.shape == probs.shape and grads.dtype == torch.float32 and grads.is_contiguous() and grads.device == probs.device)
    # c_ctc = -1  ->  grad = +gamma_ctc, exactly what the reference's kernel writes (:431-435)
    _, g, ex = loss_fwd_bwd(probs.contiguous(), labels, sizes, label_sizes, 0.0, -1.0, None, True, time_major=True,
                            blank=int(blank_label), grad_out=grads if direct else None)
    if not direct:
        grads.copy_(g)
    costs.copy_(ex["costs_ctc"].to(costs.device))


for _kv in filter(None, os.environ.get("CRF_DEBUG", "").split(",")):   # tools only (see debug_set)
    _k, _, _v = _kv.partition("=")
    try:                                                                # a stray or stale CRF_DEBUG must not break `import ctc_crf`
        debug_set(_k.strip(), int(_v) if _v.strip() else 1)
        print(f"[ctc_crf] CRF_DEBUG: switch {_k.strip()} = {_DEBUG_SET[_k.strip()]} (tools / tests only: changes product behaviour)", file=sys.stderr)
    except (ValueError, RuntimeError) as _e:
        print(f"[ctc_crf] CRF_DEBUG: ignored {_kv!r}: {_e}", file=sys.stderr)
