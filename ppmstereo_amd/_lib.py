"""ctypes binding of libppms.so (C ABI: include/ppms.h).  No CPU fallback: if the library cannot be
loaded (or built) every op raises RuntimeError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import build as _build

c_void_p, c_int, c_float, c_int64 = C.c_void_p, C.c_int, C.c_float, C.c_int64

EPI_STORE, EPI_RESID, EPI_RH, EPI_GRU, EPI_ADDF32 = range(5)
ATTN_P_BF16, ATTN_P_FP16 = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_TANH, ACT_ELU1 = range(6)


def vt_image(v: torch.Tensor, p_format: int) -> torch.Tensor:
    """The 16-bit storage of ppms_mem_attn's transposed value operand for `p_format` (include/ppms.h), as a bfloat16-typed tensor:
    bf16(v) itself, or -- ATTN_P_FP16 -- the fp16 numbers equal to those bf16 values (saturated at +-65504), bit-cast.  What the
    to_v convolution's epilogue writes with ppms_epilogue.vt_f16; callers that build V^T themselves (tests, other hosts) use this."""
    b = v.to(torch.bfloat16)
    if p_format == ATTN_P_BF16:
        return b.contiguous()
    return b.float().clamp(-65504.0, 65504.0).to(torch.float16).contiguous().view(torch.bfloat16)


def vt_values(vt: torch.Tensor, p_format: int) -> torch.Tensor:
    """fp32 values held by a V^T storage tensor (inverse of vt_image)."""
    return vt.float() if p_format == ATTN_P_BF16 else vt.view(torch.float16).float()


class SP(C.Structure):
    """ppms_sp: channel-last split-bf16 view."""
    _fields_ = [("hi", c_void_p), ("lo", c_void_p), ("ld", C.c_int32), ("c", C.c_int32)]


class Epilogue(C.Structure):
    _fields_ = [("kind", C.c_int32), ("act", C.c_int32), ("scale", c_float), ("n_valid", C.c_int32),
                ("out_sp", SP), ("out_f32", c_void_p), ("out_f32_ld", C.c_int32), ("vt_f16", C.c_int32), ("out_vt", c_void_p),
                ("aux_sp", SP), ("aux_f32", c_void_p), ("aux_f32_ld", C.c_int32), ("pre_f32_ld", C.c_int32),
                ("pre_f32", c_void_p)]


class Conv(C.Structure):
    _fields_ = [("seg", SP * 2), ("nseg", C.c_int32), ("groups", C.c_int32), ("w", c_void_p), ("bias", c_void_p),
                ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("kt", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("M", C.c_int32), ("m_split", C.c_int32), ("t_halo", C.c_int32), ("lo_zero_from", C.c_int32), ("epi", Epilogue * 2)]


class ChainLayer(C.Structure):
    _fields_ = [("w", c_void_p), ("bias", c_void_p), ("post_s", c_void_p), ("post_t", c_void_p),
                ("M", C.c_int32), ("n_valid", C.c_int32), ("resid", C.c_int32)]


class ChainParams(C.Structure):
    _fields_ = [("inp", SP), ("out", SP), ("layer", ChainLayer * 3), ("nlayers", C.c_int32), ("P", C.c_int64)]


class YUVView(C.Structure):
    """ppms_yuv_view: one view's decoded 4:2:0 frames (device pointers, byte strides)."""
    _fields_ = [("y", c_void_p), ("u", c_void_p), ("v", c_void_p), ("frame_stride_y", c_int64), ("frame_stride_c", c_int64),
                ("pitch_y", C.c_int32), ("pitch_c", C.c_int32), ("step_c", C.c_int32), ("reserved", C.c_int32)]


class YUVMatrix(C.Structure):
    """ppms_yuv_matrix: the fixed-point YCbCr -> RGB conversion."""
    _fields_ = [(n, C.c_int32) for n in ("y_off", "cy", "crv", "cgu", "cgv", "cbu", "shift", "reserved")]


class YUVFormat(C.Structure):
    """ppms_yuv_format: how ppms_video_ingest_yuv reads a view's samples (width, depth, alignment in the word, chroma subsampling)."""
    _fields_ = [(n, C.c_int32) for n in ("sample_bytes", "depth", "lsb", "sub_x", "sub_y")] + [("reserved", C.c_int32 * 3)]


class RawView(C.Structure):
    """ppms_raw_view: one view's raw sensor frames (device pointer, byte strides)."""
    _fields_ = [("data", c_void_p), ("frame_stride", c_int64), ("pitch", C.c_int32), ("reserved", C.c_int32)]


class RawFormat(C.Structure):
    """ppms_raw_format: how ppms_video_ingest_raw reads a view's samples (width, depth, alignment in the word, mosaic, black level, white balance)."""
    _fields_ = [(n, C.c_int32) for n in ("sample_bytes", "depth", "lsb", "pattern", "black")] + [("gain", C.c_int32 * 3), ("shift", C.c_int32),
                                                                                                  ("reserved", C.c_int32 * 3)]


class PackedView(C.Structure):
    """ppms_packed_view: one view's frames inside a packed surface (device pointer, byte strides, the surface column of the view's column 0)."""
    _fields_ = [("data", c_void_p), ("frame_stride", c_int64), ("pitch", C.c_int32), ("x0", C.c_int32)]


class YUVPackedFormat(C.Structure):
    """ppms_yuv_packed_format: how ppms_video_ingest_yuv_packed reads a row's components (container, depth, alignment in the word, order)."""
    _fields_ = [(n, C.c_int32) for n in ("container", "depth", "lsb", "order")] + [("reserved", C.c_int32 * 4)]


class RawPackedFormat(C.Structure):
    """ppms_raw_packed_format: how ppms_video_ingest_raw_packed reads a row's samples (packing, depth, mosaic, black level, white balance)."""
    _fields_ = [(n, C.c_int32) for n in ("packing", "depth", "pattern", "black")] + [("gain", C.c_int32 * 3), ("shift", C.c_int32),
                                                                                    ("reserved", C.c_int32 * 4)]


class RGBPackedFormat(C.Structure):
    """ppms_rgb_packed_format: how ppms_video_ingest_rgb_packed reads a pixel's channels (container, depth, alignment in the word, components per
    pixel, where R, G and B lie among them)."""
    _fields_ = [(n, C.c_int32) for n in ("container", "depth", "lsb", "step")] + [("offset", C.c_int32 * 3), ("reserved", C.c_int32)]


class RemapView(C.Structure):
    """ppms_remap_view: one view's fixed-point rectification map (device pointers, pitch in map pixels, the source frame size)."""
    _fields_ = [("xy", c_void_p), ("frac", c_void_p), ("pitch", C.c_int32), ("hs", C.c_int32), ("ws", C.c_int32),
                ("border", C.c_int32), ("fill", C.c_int32), ("reserved", C.c_int32)]


BORDER_REPLICATE, BORDER_CONSTANT = 0, 1
FMT_F32, FMT_F16, FMT_U16, FMT_U8, FMT_RGBA8, FMT_BGRA8 = range(6)       # (the last two: 4-byte colour pixels, the colour planes only)


class EgressPlane(C.Structure):
    """ppms_egress_plane: one output plane of ppms_disparity_egress (device pointer, byte strides, FMT_*)."""
    _fields_ = [("ptr", c_void_p), ("frame_stride", c_int64), ("pitch", c_int64), ("format", C.c_int32), ("reserved", C.c_int32)]


class Egress(C.Structure):
    """ppms_egress: the planes and the four conversion constants."""
    _fields_ = [("disparity", EgressPlane), ("depth", EgressPlane), ("uncertainty", EgressPlane),
                ("disp_scale", c_float), ("fb", c_float), ("depth_scale", c_float), ("min_disp", c_float)]


class Egress3D(C.Structure):
    """ppms_egress3d: a ppms_egress, the points plane, the reprojection matrix (row major), the two gates (+inf: off), 3 or 4 components."""
    _fields_ = [("base", Egress), ("points", EgressPlane), ("q", c_float * 16), ("max_uncertainty", c_float), ("max_depth", c_float),
                ("points_components", C.c_int32), ("reserved", C.c_int32)]


class Cloud(C.Structure):
    """ppms_cloud: the compact cloud's destinations (records, optional pixel indices, counts), its workspace, Q, min_disp, the gates and format."""
    _fields_ = [("records", c_void_p), ("frame_stride", c_int64), ("capacity", c_int64), ("index", c_void_p), ("index_frame_stride", c_int64),
                ("counts", c_void_p), ("block_counts", c_void_p), ("block_counts_len", c_int64), ("q", c_float * 16), ("min_disp", c_float),
                ("max_uncertainty", c_float), ("max_depth", c_float), ("format", C.c_int32), ("components", C.c_int32), ("reserved", C.c_int32)]


class Normals(C.Structure):
    """ppms_normals: the normals plane (3 elements per pixel), Q, min_disp, the two gates and the jump gate (+inf: off)."""
    _fields_ = [("normals", EgressPlane), ("q", c_float * 16), ("min_disp", c_float), ("max_uncertainty", c_float), ("max_depth", c_float),
                ("max_jump", c_float), ("reserved", C.c_int32)]


_SIGS = {
    "ppms_version": (c_int, []),
    "ppms_last_error": (C.c_char_p, []),
    "ppms_device_info": (c_int, [C.c_char_p, c_int, C.POINTER(c_int), C.POINTER(c_int)]),
    "ppms_corr_build": (c_int, [c_void_p, c_void_p, C.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_corr_lookup": (c_int, [C.POINTER(c_void_p), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_conv_gemm2": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p]),
    "ppms_conv_gemm2_slices": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_gemm2_slice_workspace_bytes": (C.c_int64, [C.POINTER(Conv), c_int]),
    "ppms_conv_gemm2_sliced": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p, c_void_p]),
    "ppms_conv_gemm2_ysweep_slices": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_gemm2_ysweep": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p, c_void_p]),
    "ppms_gemm1_applicable": (c_int, [C.POINTER(Conv)]),
    "ppms_gemm1": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p]),
    "ppms_conv_stream_applicable": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_stream": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p]),
    "ppms_conv_gemm5_applicable": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_gemm5": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_void_p]),
    "ppms_conv_gemm6_applicable": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_gemm6": (c_int, [C.POINTER(Conv), c_void_p, c_void_p]),
    "ppms_conv_gemm5_slices": (c_int, [C.POINTER(Conv)]),
    "ppms_conv_gemm5_sliced": (c_int, [C.POINTER(Conv), c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ppms_struct_sizes": (c_int, [C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int)]),
    "ppms_dwconv_gelu": (c_int, [SP, SP, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_flow_patch7": (c_int, [c_void_p, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_unc_tail": (c_int, [SP, c_void_p, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ppms_nchw_to_sp": (c_int, [c_void_p, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_sp_to_nchw": (c_int, [SP, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_nchw_to_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_nhwc_to_nchw": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_f32_to_sp": (c_int, [c_void_p, c_int, SP, c_int64, c_void_p]),
    "ppms_sp_to_f32": (c_int, [SP, c_void_p, c_int, c_int64, c_void_p]),
    "ppms_tap_gather_sum": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_flow_add": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    "ppms_convex_upsample": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_convex_upsample_3d": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_bilinear": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "ppms_disparity_egress": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(Egress), c_void_p]),
    "ppms_egress_struct_size": (c_int, []),
    "ppms_scene_egress": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(Egress3D), c_void_p]),
    "ppms_egress3d_struct_size": (c_int, []),
    "ppms_cloud_egress": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(Cloud), c_void_p]),
    "ppms_cloud_egress_workspace": (c_int64, [c_int, c_int, c_int]),
    "ppms_cloud_struct_size": (c_int, []),
    "ppms_sp_resize_blend": (c_int, [SP, SP, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p]),
    "ppms_avgpool": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_axpby": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_float, c_int64, c_int64, c_void_p]),
    "ppms_ctx_mix": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ppms_img_s2d": (c_int, [c_void_p, SP, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_yuv_struct_sizes": (c_int, [C.POINTER(c_int), C.POINTER(c_int)]),
    "ppms_remap_struct_size": (c_int, [C.POINTER(c_int)]),
    "ppms_yuv_format_struct_size": (c_int, [C.POINTER(c_int)]),
    "ppms_raw_struct_sizes": (c_int, [C.POINTER(c_int), C.POINTER(c_int)]),
    "ppms_packed_struct_sizes": (c_int, [C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int)]),
    "ppms_rgb_packed_struct_size": (c_int, [C.POINTER(c_int)]),
    "ppms_dwconv": (c_int, [SP, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_layernorm_any": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, SP, c_int64, c_int, c_void_p]),
    "ppms_grn_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "ppms_grn": (c_int, [c_void_p, c_int, c_void_p, c_void_p, SP, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ppms_sp_upsample2": (c_int, [SP, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_sp_s2d": (c_int, [SP, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_instnorm_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "ppms_instnorm_stats": (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.c_float, c_void_p, c_void_p, c_void_p]),
    "ppms_instnorm_apply": (c_int, [c_void_p, c_int, c_void_p, SP, c_int, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_qk_similarity": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_qk_pool": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_qk_cos": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ppms_qam_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ppms_attn_prep_q": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ppms_attn_prep_k": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ppms_pick_prep_k": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_int, c_int, c_void_p]),
    "ppms_pwchain": (c_int, [c_void_p, c_int64, c_void_p]),
    "ppms_pwchain_param_bytes": (c_int, []),
    "ppms_time_attn": (c_int, [SP, c_void_p, c_void_p, SP, c_int, c_int, c_int, c_void_p]),
    "ppms_layernorm": (c_int, [c_void_p, c_int, c_void_p, c_void_p, SP, SP, c_int64, c_int, c_void_p]),
    "ppms_linear_attention_workspace_floats": (c_int64, [c_int, c_int, c_int, c_int]),
    "ppms_linear_attention": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, SP, c_int, c_int, c_int, c_int, c_void_p]),
    "ppms_mem_attn": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, SP, SP, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "ppms_mem_attn_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "ppms_mem_attn_splits": (c_int, [c_int, c_int, c_int, c_int]),
    "ppms_attn_redo_accumulate": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}
# the 14 ingest entry points: ppms_video_ingest_<door>(head, tail) and its _remap twin, which takes the two views' maps between head and tail
_INGEST_HEADS = {
    "u8": [c_void_p, c_void_p, c_int64],
    "yuv420": [C.POINTER(YUVView), C.POINTER(YUVView), C.POINTER(YUVMatrix)],
    "yuv": [C.POINTER(YUVView), C.POINTER(YUVView), C.POINTER(YUVMatrix), C.POINTER(YUVFormat)],
    "raw": [C.POINTER(RawView), C.POINTER(RawView), C.POINTER(RawFormat)],
    "yuv_packed": [C.POINTER(PackedView), C.POINTER(PackedView), C.POINTER(YUVMatrix), C.POINTER(YUVPackedFormat)],
    "raw_packed": [C.POINTER(PackedView), C.POINTER(PackedView), C.POINTER(RawPackedFormat)],
    "rgb_packed": [C.POINTER(PackedView), C.POINTER(PackedView), C.POINTER(RGBPackedFormat)],
}
_INGEST_TAIL = [c_int] * 7 + [c_void_p, SP, SP, c_void_p]       # N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream
for _door, _head in _INGEST_HEADS.items():
    _SIGS["ppms_video_ingest_" + _door] = (c_int, _head + _INGEST_TAIL)
    _SIGS["ppms_video_ingest_" + _door + "_remap"] = (c_int, _head + [C.POINTER(RemapView)] * 2 + _INGEST_TAIL)
# colour out: the same 14 doors (ppms_video_colour_<door>[_remap]) with one tail, and the coloured compact cloud (ppms_cloud_egress's list + the plane)
_COLOUR_TAIL = [c_int] * 9 + [c_void_p, C.POINTER(EgressPlane), c_void_p]       # N, H0, W0, frame0, n_frames, x0, y0, h0, w0, table, out, stream
for _door, _head in _INGEST_HEADS.items():
    _SIGS["ppms_video_colour_" + _door] = (c_int, _head + _COLOUR_TAIL)
    _SIGS["ppms_video_colour_" + _door + "_remap"] = (c_int, _head + [C.POINTER(RemapView)] * 2 + _COLOUR_TAIL)
_SIGS["ppms_cloud_egress_colour"] = (c_int, _SIGS["ppms_cloud_egress"][1][:-1] + [C.POINTER(EgressPlane), c_void_p])
# normals out: the plane's launch (ppms_cloud_egress's list with its own struct) and the oriented compact cloud (that list + the normals and colour planes)
_SIGS["ppms_normals_egress"] = (c_int, _SIGS["ppms_cloud_egress"][1][:-2] + [C.POINTER(Normals), c_void_p])
_SIGS["ppms_normals_struct_size"] = (c_int, [])
_SIGS["ppms_cloud_egress_normals"] = (c_int, _SIGS["ppms_cloud_egress"][1][:-1] + [C.POINTER(EgressPlane), C.POINTER(EgressPlane), c_void_p])
_SIGS["ppms_cloud_egress_normals_workspace"] = (c_int64, [c_int, c_int, c_int])
EXPORTS = tuple(_SIGS)

# (the export that reports sizeof of the structs, their ctypes twins, the message when they differ).  An export takes one int* per struct; one
# without parameters (a single struct) returns the size.
_STRUCT_SIZES = (
    ("ppms_struct_sizes", (SP, Epilogue, Conv), "ctypes struct layout differs from include/ppms.h"),
    ("ppms_yuv_struct_sizes", (YUVView, YUVMatrix), "ctypes layout of ppms_yuv_view / ppms_yuv_matrix differs from include/ppms.h"),
    ("ppms_remap_struct_size", (RemapView,), "ctypes layout of ppms_remap_view differs from include/ppms.h"),
    ("ppms_yuv_format_struct_size", (YUVFormat,), "ctypes layout of ppms_yuv_format differs from include/ppms.h"),
    ("ppms_raw_struct_sizes", (RawView, RawFormat), "ctypes layout of ppms_raw_view / ppms_raw_format differs from include/ppms.h"),
    ("ppms_packed_struct_sizes", (PackedView, YUVPackedFormat, RawPackedFormat),
     "ctypes layout of ppms_packed_view / ppms_yuv_packed_format / ppms_raw_packed_format differs from include/ppms.h"),
    ("ppms_rgb_packed_struct_size", (RGBPackedFormat,), "ctypes layout of ppms_rgb_packed_format differs from include/ppms.h"),
    ("ppms_egress_struct_size", (Egress,), "ctypes layout of ppms_egress differs from include/ppms.h"),
    ("ppms_egress3d_struct_size", (Egress3D,), "ctypes layout of ppms_egress3d differs from include/ppms.h"),
    ("ppms_cloud_struct_size", (Cloud,), "ctypes layout of ppms_cloud differs from include/ppms.h"),
    ("ppms_normals_struct_size", (Normals,), "ctypes layout of ppms_normals differs from include/ppms.h"),
    ("ppms_pwchain_param_bytes", (ChainParams,), "ChainParams layout differs from pwchain.hip"),
)

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    return _build.LIB


def load() -> C.CDLL:
    """Load (building first if the .so is absent or stale).  Raises RuntimeError when that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        path = _build.build(verbose=not os.path.exists(_build.LIB))
        lib = C.CDLL(path)
    except Exception as exc:  # noqa: BLE001
        raise RuntimeError(f"ppmstereo_amd: the HIP library libppms.so is missing and could not be built ({exc}); "
                           "there is no CPU fallback") from exc
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.ppms_version() != 4:
        raise RuntimeError("ppmstereo_amd: libppms.so ABI version mismatch")
    for export, structs, message in _STRUCT_SIZES:
        if _SIGS[export][1]:
            sizes = [c_int() for _ in structs]
            getattr(lib, export)(*(C.byref(x) for x in sizes))
            sizes = [x.value for x in sizes]
        else:
            sizes = [getattr(lib, export)()]
        if sizes != [C.sizeof(t) for t in structs]:
            raise RuntimeError("ppmstereo_amd: " + message)
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("libppms: " + load().ppms_last_error().decode())


def stream_ptr() -> int:
    """hipStream_t of torch's current stream (kernels are enqueued there; nothing synchronises)."""
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ppmstereo_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class SPTensor:
    """Owner of a split-bf16 channel-last activation: data (2, before + P + after, ld) bf16; views select a channel range of
    the P "own" pixels.  before / after: extra pixel rows around them -- the temporal halo slabs of a frame-sharded window
    (ppmstereo_amd/dist.py) or, for gathered tensors, the other ranks' frames."""

    def __init__(self, pixels: int, channels: int, device, zero: bool = True, before: int = 0, after: int = 0):
        alloc = torch.zeros if zero else torch.empty
        self.data = alloc((2, before + pixels + after, channels), dtype=torch.bfloat16, device=device)
        self.pixels, self.channels, self.before, self.after = pixels, channels, before, after

    def view(self, c0: int = 0, c: Optional[int] = None, all_rows: bool = False) -> SP:
        """SP view of channels [c0, c0 + c) starting at the first own pixel (all_rows: at the first allocated row)."""
        c = self.channels - c0 if c is None else c
        assert 0 <= c0 and c0 + c <= self.channels
        total = self.before + self.pixels + self.after
        base = self.data.data_ptr() + (0 if all_rows else self.before) * self.channels * 2
        plane = total * self.channels * 2
        return SP(base + c0 * 2, base + plane + c0 * 2, self.channels, c)

    def own(self) -> torch.Tensor:
        """(2, P, ld) view of the own pixels."""
        return self.data[:, self.before:self.before + self.pixels]

    def to_f32(self, c0: int = 0, c: Optional[int] = None) -> torch.Tensor:
        """(P, c) fp32 = hi + lo of the own pixels (torch ops; for tests and glue)."""
        c = self.channels - c0 if c is None else c
        d = self.own()
        return d[0, :, c0:c0 + c].float() + d[1, :, c0:c0 + c].float()

    def set_f32(self, x: torch.Tensor, c0: int = 0) -> None:
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
        d = self.own()
        d[0, :, c0:c0 + x.shape[1]] = hi
        d[1, :, c0:c0 + x.shape[1]] = lo
