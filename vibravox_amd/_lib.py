"""ctypes binding of ``libeben_hip.so`` (C ABI declared in ``include/eben_hip.h``).

There is deliberately NO fallback: if the shared library is missing, or a tensor handed to an
op is not a contiguous float32 tensor on a HIP device, the call raises.  The CPU oracle under
``oracle/`` is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libeben_hip.so")


class EbenError(RuntimeError):
    pass


class EbenConv1dDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32),
        ("c_in", c_int32),
        ("c_out", c_int32),
        ("l_in", c_int32),
        ("l_out", c_int32),
        ("ksize", c_int32),
        ("stride", c_int32),
        ("dilation", c_int32),
        ("groups", c_int32),
        ("pad_l", c_int32),
        ("pad_r", c_int32),
        ("pad_mode", c_int32),
        ("transposed", c_int32),
        ("in_slope", c_float),
        ("out_slope", c_float),
        ("math", c_int32),
    ]


class EbenPackJob(ctypes.Structure):
    _fields_ = [("desc", EbenConv1dDesc), ("v", c_void_p), ("scale", c_void_p), ("wp_fwd", c_void_p), ("wp_bwd", c_void_p)]


class EbenRuPackJob(ctypes.Structure):
    _fields_ = [("channels", c_int32), ("math", c_int32), ("which", c_int32), ("pad_", c_int32),
                ("v_dil", c_void_p), ("scale_dil", c_void_p), ("v_pw", c_void_p), ("scale_pw", c_void_p), ("wimg", c_void_p)]


class EbenWnScaleItem(ctypes.Structure):
    _fields_ = [("g", c_void_p), ("v", c_void_p), ("scale", c_void_p), ("norm", c_void_p), ("rows", c_int32), ("cols", c_int32)]


class EbenWnBwdItem(ctypes.Structure):
    _fields_ = [("slabs", c_void_p), ("g", c_void_p), ("v", c_void_p), ("norm", c_void_p), ("dg", c_void_p), ("dv", c_void_p),
                ("dbias", c_void_p), ("slab_stride", c_int64), ("nslab", c_int32), ("rows", c_int32), ("cols", c_int32),
                ("row_stride", c_int32), ("col_perm_k", c_int32), ("pad_", c_int32)]


class EbenBlHeadJob(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("v", c_void_p), ("scale", c_void_p), ("bias", c_void_p), ("y_hi", c_void_p), ("y_lo", c_void_p),
                ("c_in", c_int32), ("c_out", c_int32), ("l_in", c_int32), ("l_out", c_int32), ("ksize", c_int32), ("dilation", c_int32),
                ("pad", c_int32), ("reflect_pad", c_int32), ("out_slope", c_float), ("pad_", c_int32)]


class EbenAdamTensor(ctypes.Structure):
    _fields_ = [
        ("param", c_void_p),
        ("grad", c_void_p),
        ("exp_avg", c_void_p),
        ("exp_avg_sq", c_void_p),
        ("numel", c_int64),
    ]


class EbenCollateItem(ctypes.Structure):
    _fields_ = [("speech", c_void_p), ("airborne", c_void_p), ("noise", c_void_p), ("length", c_int64), ("noise_start", c_int64),
                ("shift", c_int64)]


class EbenCopySegment(ctypes.Structure):
    _fields_ = [("dst", c_void_p), ("src", c_void_p), ("floats", c_int64)]


RATE_MAX_SPLICES, RATE_MAX_PIECES, RATE_MAX_RATIOS = 64, 128, 8   # EBEN_RATE_MAX_SPLICES / _PIECES descriptors a call, EBEN_RATE_MAX_RATIOS


class EbenRateSplice(ctypes.Structure):
    _fields_ = [(k, c_int) for k in ("slot", "src_row", "prev_off", "n_carry", "n_new", "tape")]


class EbenRateRatio(ctypes.Structure):
    _fields_ = [("kernels", c_void_p), ("orig", c_int), ("nw", c_int), ("width", c_int), ("reserved", c_int)]


class EbenRatePiece(ctypes.Structure):
    _fields_ = [(k, c_int) for k in ("len", "p0", "base0", "n_out", "end", "first_out")] + [(k, ctypes.c_uint8) for k in ("slot", "ratio", "tape", "fifo")]


PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 0, 1, 2, 3   # EBEN_PCM_*


class EbenPcmRow(ctypes.Structure):
    _fields_ = [("byte_offset", c_int64), ("frames", c_int32), ("channels", c_int32), ("channel", c_int32), ("format", c_int32)]


class EbenPcmEncRow(ctypes.Structure):
    _fields_ = [("src_offset", c_int64), ("byte_offset", c_int64), ("samples", c_int32), ("format", c_int32)]


STREAM_PCM_MAX_PIECES, PCM_MAX_CHUNKS, PCM_CHUNK_TILE = 64, 64, 1024   # EBEN_STREAM_PCM_MAX_PIECES, EBEN_PCM_MAX_CHUNKS, EBEN_PCM_CHUNK_TILE


class EbenStreamPcmPiece(ctypes.Structure):
    _fields_ = ([(k, c_int) for k in ("prev_off", "n_carry", "n_new", "p0", "base0", "n_out", "byte_offset")] + [("src_row", ctypes.c_uint16)]
                + [(k, ctypes.c_uint8) for k in ("slot", "tape")] + [("ratio", ctypes.c_int8)] + [(k, ctypes.c_uint8) for k in ("format", "end", "reserved")])


class EbenPcmChunk(ctypes.Structure):
    _fields_ = [("bytes", c_void_p), ("n", c_int32), ("format", c_int32), ("dst_row", c_int32)]


class EbenPackEntry(ctypes.Structure):
    _fields_ = [("tensor", c_void_p), ("image_offset", c_int64), ("nbytes", c_int64), ("kind", c_int32), ("reserved", c_int32)]


class EbenClip(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("length", c_int64)]


CLIP_MAX_BANDS = 16   # EBEN_CLIP_MAX_BANDS ratios a call of eben_resample_clips


class EbenClipBand(ctypes.Structure):
    _fields_ = [("band", c_void_p), ("first", c_void_p), ("orig", c_int32), ("nw", c_int32), ("width", c_int32), ("W", c_int32)]


class EbenResampleClip(ctypes.Structure):
    _fields_ = [("src_offset", c_int64), ("t_in", c_int32), ("band", c_int32), ("dst_row", c_int32), ("reserved", c_int32)]


class EbenVocoderClip(ctypes.Structure):
    _fields_ = [("rate", ctypes.c_double), ("frames_out", c_int32), ("col_out", c_int32)]


class EbenOlaClip(ctypes.Structure):
    _fields_ = [("dst_offset", c_int64), ("col", c_int32), ("frames_out", c_int32), ("len_stretch", c_int32), ("valid", c_int32)]


class EbenMaskClip(ctypes.Structure):
    _fields_ = [("row", c_int32), ("first", c_int32), ("count", c_int32)]


_P = c_void_p
_D = POINTER(EbenConv1dDesc)

# name -> (restype, argtypes); mirrors include/eben_hip.h one to one
SIGNATURES = {
    "eben_last_error": (c_char_p, []),
    "eben_version": (c_int, []),
    "eben_device_info": (c_int, [ctypes.c_char_p, c_size_t]),
    "eben_wn_scale": (c_int, [_P, _P, c_int, c_int, _P, _P, _P]),
    "eben_wn_bwd": (c_int, [_P, c_int, c_size_t, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "eben_wn_scale_multi": (c_int, [POINTER(EbenWnScaleItem), c_int, _P]),
    "eben_wn_bwd_multi": (c_int, [POINTER(EbenWnBwdItem), c_int, _P]),
    "eben_conv1d_packed_floats": (c_size_t, [_D, c_int]),
    "eben_conv1d_kernel_generation": (c_int, [_D, c_int]),
    "eben_conv1d_variant": (c_int, [_D, c_int, c_int, POINTER(c_int), c_int]),
    "eben_conv1d_variant_f32": (c_int, [_D, c_int, c_int, POINTER(c_int), c_int]),
    "eben_conv1d_pack": (c_int, [_D, _P, _P, _P, _P, _P]),
    "eben_conv1d_pack_multi": (c_int, [POINTER(EbenPackJob), c_int, _P]),
    "eben_conv1d_fwd": (c_int, [_D, _P, _P, _P, _P, _P, _P]),
    "eben_conv1d_fwd_res": (c_int, [_D, _P, _P, _P, _P, c_float, _P, _P]),
    "eben_conv1d_bwd_dx_res": (c_int, [_D, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "eben_conv1d_bwd_dx_workspace": (c_size_t, [_D]),
    "eben_conv1d_bwd_dw_workspace": (c_size_t, [_D, POINTER(c_int), POINTER(c_int)]),
    "eben_conv1d_bwd_dx": (c_int, [_D, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "eben_conv1d_bwd_dx_ex": (c_int, [_D, _P, _P, _P, c_int, _P, c_float, c_int, POINTER(c_int), _P, _P]),
    "eben_conv1d_bwd_dx_fm": (c_int, [_D, _P, _P, _P, c_int, _P, c_float, _P, c_float, c_int, POINTER(c_int), _P, _P]),
    "eben_conv1d_bwd_dw": (c_int, [_D, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "eben_conv1d_bwd_dw_variant": (c_int, [_D, POINTER(c_int), c_int]),
    "eben_conv1d_bwd_dw_f32_variant": (c_int, [_D, POINTER(c_int), c_int]),
    "eben_bl_from_f32": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "eben_bl_to_f32": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P]),
    "eben_bl_conv1d_fwd": (c_int, [_D, _P, _P, _P, _P, _P, _P, _P]),
    "eben_bl_conv1d_bwd_dx": (c_int, [_D, _P, _P, _P, _P, c_float, c_int, POINTER(c_int), c_int, c_int, _P, c_float, _P, _P, _P]),
    "eben_bl_dx_pr_desc": (c_int, [_D, _D]),
    "eben_bl_dx_pr_weights": (c_int, [_D, _P, _P, _P, _P]),
    "eben_bl_conv1d_bwd_dx_pr": (c_int, [_D, _P, _P, _P, _P, c_float, c_int, POINTER(c_int), c_int, c_int, _P, c_float, _P, _P, _P]),
    "eben_bl_conv1d_bwd_dx_c": (c_int, [_D, _P, _P, _P, _P, _P, c_float, c_int, POINTER(c_int), c_int, c_int, _P, c_float, _P, _P, _P]),
    "eben_bl_conv1d_bwd_dx_pr_c": (c_int, [_D, _P, _P, _P, _P, _P, c_float, c_int, POINTER(c_int), c_int, c_int, _P, c_float, _P, _P, _P]),
    "eben_bl_conv1d_bwd_dw_workspace": (c_size_t, [_D, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "eben_bl_conv1d_bwd_dw": (c_int, [_D, _P, _P, c_int, _P, c_size_t, _P]),
    "eben_bl_conv1d_bwd_dw_multi": (c_int, [POINTER(_D), POINTER(_P), POINTER(_P), c_int, POINTER(_P), POINTER(c_size_t), c_int, _P]),
    "eben_bl_conv1d_bwd_dw_variant": (c_int, [_D, POINTER(c_int), c_int]),
    "eben_bl_head_fwd": (c_int, [POINTER(EbenBlHeadJob), c_int, c_int, _P]),
    "eben_bl_head_dx": (c_int, [POINTER(EbenBlHeadJob), c_int, c_int, _P, _P]),
    "eben_bl_head_dw_workspace": (c_size_t, [POINTER(EbenBlHeadJob), c_int, POINTER(c_int), POINTER(c_int)]),
    "eben_bl_head_dw": (c_int, [POINTER(EbenBlHeadJob), c_int, _P, c_size_t, _P]),
    "eben_bl_tail_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_float, _P, _P]),
    "eben_bl_tail_dx": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_float, c_int, POINTER(c_int), c_int, c_int, _P, c_float,
                                _P, _P, _P]),
    "eben_bl_tail_dw_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "eben_bl_tail_dw": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "eben_bl_fm_sums_workspace": (c_size_t, [c_int]),
    "eben_bl_fm_sums": (c_int, [POINTER(c_void_p), POINTER(c_int64), c_int, _P, c_size_t, _P, _P]),
    "eben_bl_fm_sums_codes": (c_int, [POINTER(c_void_p), POINTER(c_int64), POINTER(c_void_p), c_int, _P, c_size_t, _P, _P]),
    "eben_ru_packed_floats": (c_size_t, [c_int]),
    "eben_ru_pack": (c_int, [c_int, _P, _P, _P, _P, _P, _P]),
    "eben_ru_fwd": (c_int, [c_int, c_int, c_int, c_int, _P, c_float, c_float, _P, _P, _P, _P, _P]),
    "eben_ru_pack_bwd": (c_int, [c_int, _P, _P, _P, _P, _P, _P]),
    "eben_ru_bwd": (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_float, _P, c_float, _P, _P, _P, _P, _P]),
    "eben_ru_packed_floats_ex": (c_size_t, [c_int, c_int]),
    "eben_ru_supported": (c_int, [c_int, c_int, c_int]),
    "eben_ru_pack_ex": (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "eben_ru_pack_multi": (c_int, [POINTER(EbenRuPackJob), c_int, _P]),
    "eben_ru_fwd_ex": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, c_float, c_float, _P, _P, _P, _P, _P]),
    "eben_ru_bwd_ex": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, _P, c_float, _P, c_float, _P, _P, _P, _P, _P]),
    "eben_ru_dw_slabs": (c_int, [c_int, c_int, c_int]),
    "eben_ru_dw": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, _P, c_float, _P, _P, _P, c_float, _P, _P, _P]),
    "eben_rubl_supported": (c_int, [c_int, c_int]),
    "eben_rubl_fwd": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "eben_rubl_bwd": (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_float, _P, c_float, _P, _P, _P, _P, _P, _P]),
    "eben_rubl_dw_slabs": (c_int, [c_int, c_int, c_int]),
    "eben_rubl_dw": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "eben_ru_variant": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_int]),
    "eben_fir_decimate": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_fir_interp_sum": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_fir_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int), c_int]),
    "eben_lrelu_fwd": (c_int, [_P, _P, c_size_t, c_float, _P]),
    "eben_lrelu_bwd": (c_int, [_P, _P, _P, c_size_t, c_float, _P]),
    "eben_space_to_depth": (c_int, [_P, _P, c_float, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_gemm_packed_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "eben_gemm_pack": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P]),
    "eben_gemm_fwd": (c_int, [c_int, c_int, c_int, c_int, ctypes.c_longlong, _P, _P, _P, _P]),
    "eben_add": (c_int, [_P, _P, _P, c_size_t, _P]),
    "eben_axpby": (c_int, [_P, c_float, _P, c_float, _P, c_size_t, _P]),
    "eben_tanh_lift_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "eben_tanh_bwd": (c_int, [_P, _P, _P, c_size_t, _P]),
    "eben_reflect_pad_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "eben_reflect_pad_bwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "eben_fm_sums": (c_int, [POINTER(c_void_p), POINTER(c_int64), c_int, _P, c_size_t, _P, _P]),
    "eben_fm_sums_workspace": (c_size_t, [c_int]),
    "eben_fm_bwd": (c_int, [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64), c_int, _P, _P, c_float, _P]),
    "eben_hinge_fwd": (c_int, [_P, c_size_t, c_float, _P, _P]),
    "eben_hinge_fwd_multi": (c_int, [POINTER(c_void_p), POINTER(c_int64), POINTER(c_float), c_int, _P, _P]),
    "eben_disc_losses": (c_int, [_P, c_int, c_float, _P, c_int, _P, _P]),
    "eben_stft_loss_total": (c_int, [POINTER(c_void_p), POINTER(c_float), c_int, c_int, _P, _P]),
    "eben_last_conv_norms_workspace": (c_size_t, [c_int]),
    "eben_last_conv_norms": (c_int, [POINTER(c_void_p), c_int, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P, _P]),
    "eben_balance": (c_int, [POINTER(c_void_p), POINTER(c_void_p), c_int, _P, c_int, c_int, c_float, c_float, _P, _P, _P]),
    "eben_weighted_sum": (c_int, [POINTER(c_void_p), _P, c_int, c_size_t, _P, _P]),
    "eben_hinge_bwd": (c_int, [_P, c_size_t, c_float, _P, c_float, _P, _P]),
    "eben_hinge_bwd_stacked": (c_int, [_P, _P, c_size_t, _P, c_float, c_float, c_float, _P, _P]),
    "eben_stft_loss_sums_workspace": (c_size_t, [c_int]),
    "eben_time_mask": (c_int, [_P, c_int64, c_int, c_int, c_int, _P]),
    "eben_phase_vocoder": (c_int, [_P, _P, c_int, c_int, c_int, c_int, ctypes.c_double, c_float, _P]),
    "eben_resample": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_resample_clips": (c_int, [_P, c_int64, _P, c_int, c_int, POINTER(EbenClipBand), c_int, POINTER(EbenResampleClip), c_int, _P]),
    "eben_phase_vocoder_clips": (c_int, [_P, _P, c_int, c_int, c_int64, POINTER(EbenVocoderClip), c_int, c_float, _P]),
    "eben_overlap_add_clips": (c_int, [_P, c_int64, _P, _P, c_int64, c_int, c_int, c_int, POINTER(EbenOlaClip), c_int, _P]),
    "eben_time_mask_clips": (c_int, [_P, c_int, c_int, POINTER(EbenMaskClip), c_int, _P]),
    "eben_stft_frames": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_stft_frames_folded": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_split3": (c_int, [_P, _P, c_int, c_int, c_int64, _P]),
    "eben_overlap_add_folded_tiled": (c_int, [c_int, c_int, c_int, c_int]),
    "eben_overlap_add_folded": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, _P]),
    "eben_stft_loss_sums_ex": (c_int, [_P, _P, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_float, _P, c_size_t, _P, _P]),
    "eben_stft_loss_bwd_ex": (c_int, [_P, _P, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_float, _P, _P, c_float, _P, c_int64, c_int64,
                                      c_int64, _P]),
    "eben_overlap_add_ex": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, _P]),
    "eben_stft_terms_workspace": (c_size_t, [c_int]),
    "eben_stft_terms_fwd": (c_int, [_P, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, c_int, c_int, _P, _P, c_size_t, _P, _P]),
    "eben_stft_terms_bwd": (c_int, [_P, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, c_int, c_int, c_float, c_float, c_float, _P, _P,
                                    c_float, _P, _P]),
    "eben_stft_terms_total": (c_int, [POINTER(c_void_p), POINTER(c_float), c_int, c_int, c_int, c_float, c_float, c_float, _P, _P]),
    "eben_adam_step": (c_int, [POINTER(EbenAdamTensor), c_int, c_int64, c_float, c_float, c_float, c_float, c_float, c_int, c_float, _P]),
    "eben_noisy_collate": (c_int, [POINTER(EbenCollateItem), c_int, c_int, _P, _P, _P]),
    "eben_clip_powers_workspace": (c_size_t, [c_int]),
    "eben_clip_powers": (c_int, [POINTER(EbenClip), c_int, _P, _P, c_size_t, _P]),
    "eben_noisy_collate_scaled": (c_int, [POINTER(EbenCollateItem), c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "eben_biquad_workspace": (c_size_t, [c_int, c_int]),
    "eben_biquad": (c_int, [_P, _P, c_int, c_int, c_int, POINTER(ctypes.c_double), c_int, c_int, _P, c_size_t, _P]),
    "eben_l2norm": (c_int, [_P, c_size_t, _P, _P]),
    "eben_si_sdr": (c_int, [_P, _P, c_int, c_int, _P, _P]),
    "eben_stoi_workspace": (c_size_t, [c_int, c_int, c_int]),
    "eben_stoi": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, c_size_t, _P, _P]),
    "eben_si_sdr_ragged": (c_int, [_P, _P, c_int, c_int, _P, _P, _P]),
    "eben_stoi_ragged_workspace": (c_size_t, [c_int, c_int, c_int]),
    "eben_stoi_ragged": (c_int, [_P, _P, c_int, c_int, _P, c_int, _P, c_int, _P, c_size_t, _P, _P]),
    "eben_signal_ratio": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, _P, _P]),
    "eben_estoi_workspace": (c_size_t, [c_int, c_int, c_int]),
    "eben_estoi": (c_int, [_P, _P, c_int, c_int, _P, c_int, _P, c_int, _P, c_size_t, _P, _P, _P]),
    "eben_lsd_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "eben_lsd": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, POINTER(c_int), POINTER(c_int), c_int, _P, c_size_t, _P, _P]),
    "eben_sdr_workspace": (c_size_t, [c_int, c_int, c_int]),
    "eben_sdr": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, ctypes.c_double, _P, _P, _P]),
    "eben_speech_measures_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "eben_speech_measures": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, _P, _P, _P, _P]),
    "eben_multirate_down": (c_int, [_P, _P, POINTER(c_int), POINTER(c_void_p), c_int, c_int, c_int, _P]),
    "eben_multirate_down_adjoint": (c_int, [_P, POINTER(c_void_p), _P, POINTER(c_int), _P, c_int, c_int, c_int, _P]),
    "eben_resample_adjoint": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_edge_fill": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_edge_zero": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "eben_fm_sums_rows_workspace": (c_size_t, [c_int, c_int]),
    "eben_fm_sums_rows": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_void_p), c_int, c_int, _P, c_size_t, _P, _P]),
    "eben_hinge_rows": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_float), POINTER(c_void_p), c_int, c_int, _P, _P]),
    "eben_stft_loss_sums_rows_workspace": (c_size_t, [c_int]),
    "eben_stft_loss_sums_rows": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int64, c_int64, c_int64, c_float, _P, c_size_t, _P, _P]),
    "eben_clip_losses": (c_int, [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int), c_int, _P, c_int, c_float, _P, c_int, c_int, _P, _P]),
    "eben_stream_splice": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P]),
    "eben_stream_splice_rows": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, c_int, c_int,
                                        POINTER(ctypes.c_uint64), c_int, c_int, _P]),
    "eben_copy_segments": (c_int, [POINTER(EbenCopySegment), c_int, _P]),
    "eben_resample_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int), c_int]),
    "eben_resample_ragged": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_resample_stream": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "eben_rate_splice_slots": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, POINTER(EbenRateSplice), c_int, _P]),
    "eben_resample_slots": (c_int, [_P, _P, c_int, _P, _P, c_int, c_int, POINTER(EbenRateRatio), c_int, POINTER(EbenRatePiece), c_int, _P]),
    "eben_pcm_decode_ragged": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, _P, c_int, c_int64, _P]),
    "eben_pcm_resample_ragged": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, _P, _P, c_int, c_int64, c_int, c_int, c_int, _P]),
    "eben_pcm_encode_plan": (c_int, [POINTER(c_int), c_int]),
    "eben_pcm_encode_ragged": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, c_int, _P]),
    "eben_pcm_encode_ragged_gain": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, _P, c_int, _P]),
    "eben_k_weighting": (c_int, [c_int, POINTER(ctypes.c_double)]),
    "eben_loudness_workspace": (c_size_t, [c_int, c_int, c_int]),
    "eben_loudness": (c_int, [_P, c_int, c_int, _P, c_int, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, c_size_t, _P]),
    "eben_stream_pcm_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int), c_int]),
    "eben_stream_pcm_out": (c_int, [_P, _P, c_int, c_int, _P, c_int, c_int, POINTER(EbenRateRatio), c_int, _P, c_int64, _P, POINTER(EbenStreamPcmPiece),
                                    c_int, _P]),
    "eben_pcm_chunks_in": (c_int, [POINTER(EbenPcmChunk), c_int, _P, c_int, c_int, _P]),
    "eben_pack_tensors": (c_int, [POINTER(EbenPackEntry), c_int, _P, c_int64, _P, _P]),
    "eben_unpack_tensors": (c_int, [POINTER(EbenPackEntry), c_int, _P, c_int64, _P]),
    "eben_pack_plan": (c_int, [POINTER(EbenPackEntry), c_int, POINTER(c_int64), POINTER(c_int)]),
}

_lib: Optional[ctypes.CDLL] = None


#: include/eben_hip.h EBEN_ABI_VERSION this module's structures and signatures were written against
ABI_VERSION = 6


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the library and attach the prototypes.  Works without a GPU (symbols only)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("EBEN_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise EbenError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `vibravox_amd/csrc/build.sh` (there is no CPU fallback)."
        )
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    have = lib.eben_version()
    if have != ABI_VERSION:   # a stale .so (or a caller built against another header) would mis-stride the POD tables
        raise EbenError(f"{p} reports ABI version {have}, this package binds version {ABI_VERSION} (include/eben_hip.h EBEN_ABI_VERSION): rebuild it "
                        f"with vibravox_amd/csrc/build.sh")
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().eben_last_error()
        raise EbenError(f"{what or 'libeben_hip'} failed (code {rc}): {msg.decode() if msg else '?'}")


def pcm_encode_tile() -> int:
    """Samples of one row that a block of ``eben_pcm_encode_ragged`` owns (``eben_pcm_encode_plan``; no GPU needed)."""
    out = (c_int * 1)()
    check(load().eben_pcm_encode_plan(out, 1), "pcm_encode_plan")
    return int(out[0])


def pack_block_bytes() -> int:
    """Bytes of one entry that a block of ``eben_pack_tensors`` / ``eben_unpack_tensors`` owns (``eben_pack_plan``; no GPU needed)."""
    out = c_int(0)
    check(load().eben_pack_plan(None, 0, None, ctypes.byref(out)), "pack_plan")
    return int(out.value)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a tensor the kernels may touch (contiguous float32 on a HIP device)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise EbenError(
            f"vibravox_amd ops run only on an MI355X HIP device (got a tensor on '{t.device}'); "
            "there is no CPU path -- the CPU oracle lives under oracle/ and is test-only."
        )
    if t.dtype is not torch.float32 or not t.is_contiguous():
        raise EbenError(f"expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t.data_ptr()


def stream() -> int:
    """Raw handle of torch's current HIP stream (two C calls: ~20x cheaper than torch.cuda.current_stream().cuda_stream,
    which builds a Python Stream object -- it was 2.6 ms of CPU per train step)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
