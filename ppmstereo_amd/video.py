"""Video into the model: what ``PPMStereo.forward`` / ``forward_batch_test`` accept beside the reference's float tensors (uint8 and decoded
YUV frames of 8, 10 or 12 bits with 4:2:0 / 4:2:2 / 4:4:4 chroma, a sensor's Bayer-mosaic or monochrome frames, both in the packed formats cameras put
on the wire (YUYV, Y210, v210, RAW10p / RAW12p), interleaved RGB of 8, 10 or 12 bits (BGR24, BGRA, RGB48, X2RGB10), unrectified frames with a ``StereoRectifier``), the one private family of sources that stands for all of them behind the front doors
(``stereo_source``) and the sliding-window schedule.  A source also hands the left view back as colour bytes (``colour``; ``colour_bytes`` is the
definition), for output.py's "colour" plane.  Nothing here knows the model.  (What the doors hand back: output.py.)"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib as L


class InputPadder:
    """Replicate-pads the last two dimensions up to multiples of ``divis_by`` and crops results back (the reference's helper,
    models/core/utils/utils.py:19-44).  "sintel" mode centres the image (the extra row / column of an odd pad goes to the bottom /
    right); any other mode pads the height at the bottom only."""

    def __init__(self, dims, mode: str = "sintel", divis_by: int = 8):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        extra_h, extra_w = -self.ht % divis_by, -self.wd % divis_by
        left, top = extra_w // 2, (extra_h // 2 if mode == "sintel" else 0)
        self._pad = [left, extra_w - left, top, extra_h - top]          # F.pad order: left, right, top, bottom

    def geometry(self):
        """(pad_left, pad_top, H, W): the columns / rows ``pad`` adds in front and the padded size (what ppms_video_ingest_u8 takes)."""
        left, right, top, bottom = self._pad
        return left, top, top + self.ht + bottom, left + self.wd + right

    def pad(self, *inputs):
        for x in inputs:
            if x.ndim != 4:
                raise ValueError(f"InputPadder.pad: 4-D tensors expected, got {tuple(x.shape)}")
        if not any(self._pad):
            return list(inputs)                                           # (already a multiple: nothing to copy)
        return [torch.nn.functional.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        if x.ndim != 4:
            raise ValueError(f"InputPadder.unpad: 4-D tensor expected, got {tuple(x.shape)}")
        left, right, top, bottom = self._pad
        return x[..., top:x.shape[-2] - bottom, left:x.shape[-1] - right]


_LEVEL_LUT: Dict[tuple, torch.Tensor] = {}                                   # (device index, depth) -> table
_DEPTHS = (8, 10, 12)


def _check_depth(who: str, depth) -> int:
    if depth not in _DEPTHS:
        raise ValueError(f"{who}: depth = {depth!r}; one of {_DEPTHS}")
    return int(depth)


def _levels_to_float(levels: torch.Tensor, depth: int) -> torch.Tensor:
    """RGB levels of ``depth`` bits -> the float32 video in [0, 255] that stands for them (depth 8: the bytes' values, no multiply)."""
    return levels.float() if depth == 8 else levels.float() * (255.0 / ((1 << depth) - 1))


def _cuda_index(device) -> int:
    """The index of the GPU a ``device`` argument means: "cuda" without an index is the current device."""
    index = torch.device(device).index
    return torch.cuda.current_device() if index is None else index


def _moved_to(device) -> torch.device:
    """Where ``to(device)`` of frames and maps goes: the indexed GPU of ``_cuda_index``, or the host device as it is."""
    device = torch.device(device)
    return torch.device("cuda", _cuda_index(device)) if device.type == "cuda" else device


def _sample_lsb(who: str, align, depth: int, words: bool) -> int:
    """``align`` checked, as the bit of a 16-bit word that holds the sample's lowest bit (bytes, and words read from the bottom: 0)."""
    if align not in ("msb", "lsb"):
        raise ValueError(f"{who}: align {align!r}; 'msb' or 'lsb'")
    return 16 - depth if (words and align == "msb") else 0


def _check_plane(who: str, name: str, t, dtype, dims: str = "(N, rows, columns)", depth: int = 8) -> None:
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 3:
        raise ValueError(f"{who}: {name} must be a {str(dtype).replace('torch.', '')} tensor {dims}" + ("" if depth == 8 else f" at depth {depth}"))


def _strides(t: torch.Tensor, row: int):
    """(pitch, frame stride) in elements of a plane (N, rows, .) whose rows span ``row`` elements, first to the end of the last -- or None where
    rows or frames overlap.  A size-1 dimension's stride is arbitrary: the smallest the kernel accepts stands in for it."""
    n, rows = t.shape[:2]
    pitch = t.stride(1) if rows > 1 else row
    frame = t.stride(0) if n > 1 else (rows - 1) * pitch + row
    return None if pitch < row or frame < (rows - 1) * pitch + row else (pitch, frame)


def level_lut(device, depth: int = 8) -> torch.Tensor:
    """fp32 [2^depth] on `device`: the normalised value of every RGB level of ``depth`` bits, from the expressions a level meets on the float
    path ON THE SAME DEVICE -- ``to_float``'s ``level * (255.0 / (2^depth - 1))`` (depth 8: the byte's value as it is), then ``forward``'s
    ``2 * (x / 255.0) - 1.0``.  torch's division by a Python scalar need not round like a division written elsewhere, so the table is what makes
    the decoded paths the float path's bits.  Built once per (device, depth) and kept (the host waits for it once)."""
    depth = _check_depth("level_lut", depth)
    idx = _cuda_index(device)
    if (idx, depth) not in _LEVEL_LUT:
        dev = torch.device("cuda", idx)
        x = _levels_to_float(torch.arange(1 << depth, dtype=torch.float32, device=dev), depth)
        _LEVEL_LUT[idx, depth] = (2 * (x / 255.0) - 1.0).contiguous()
        torch.cuda.current_stream(dev).synchronize()             # later calls may read it from any stream
    return _LEVEL_LUT[idx, depth]


def byte_lut(device) -> torch.Tensor:
    """fp32 [256] on `device`: the normalised value of every byte -- ``level_lut``'s depth-8 entry."""
    return level_lut(device, 8)


_COLOUR_ORDERS = {"rgba8": ((0, 1, 2), L.FMT_RGBA8), "bgra8": ((2, 1, 0), L.FMT_BGRA8)}      # order: (channels of the first three bytes, PPMS_FMT_*)
_COLOUR_LUT: Dict[tuple, torch.Tensor] = {}                                  # (device, depth) -> table


def _check_colour_order(who: str, order) -> str:
    if order not in _COLOUR_ORDERS:
        raise ValueError(f"{who}: colour order {order!r}; one of {sorted(_COLOUR_ORDERS)}")
    return order


def _to_bytes(values: torch.Tensor) -> torch.Tensor:
    """clamp(rint(values), 0, 255) as uint8: ties to even, NaN -> 0 -- the colour byte a float value in [0, 255] stands for."""
    r = torch.round(values.float())
    return torch.where(torch.isnan(r), torch.zeros_like(r), r).clamp(0.0, 255.0).to(torch.uint8)


def colour_bytes(float_left: torch.Tensor, order: str = "rgba8") -> torch.Tensor:
    """The colour plane of a float video: ``float_left`` (..., 3, H, W) in [0, 255] (a source's ``float_views()[0]``: the left view as the network is
    defined on it) -> uint8 (..., H, W, 4), per pixel R, G, B, 255 ("rgba8") or B, G, R, 255 ("bgra8": read as a little-endian uint32 0xFFRRGGBB, the
    packing of PCL's PointXYZRGB).  A byte is clamp(rint(value), 0, 255), ties to even, NaN -> 0.  The definition the colour kernels are tested
    against, and the float path's own arithmetic."""
    channels, _ = _COLOUR_ORDERS[_check_colour_order("colour_bytes", order)]
    if not torch.is_tensor(float_left) or float_left.dim() < 3 or float_left.shape[-3] != 3:
        raise ValueError(f"colour_bytes: a video (..., 3, H, W) expected, got {tuple(float_left.shape) if torch.is_tensor(float_left) else type(float_left).__name__}")
    c = _to_bytes(float_left)
    return torch.stack([c[..., i, :, :] for i in channels] + [torch.full_like(c[..., 0, :, :], 255)], dim=-1)


def colour_lut(device, depth: int = 8) -> torch.Tensor:
    """uint8 [2^depth] on ``device`` (a GPU, or the host): the colour byte of every RGB level of ``depth`` bits -- ``_to_bytes`` of the float value
    the level stands for on the float path on the same device (depth 8: the level itself).  What the colour kernel looks levels up in.  Built once
    per (device, depth) and kept (on a GPU the host waits for it once)."""
    depth = _check_depth("colour_lut", depth)
    dev = _moved_to(device)
    if (dev, depth) not in _COLOUR_LUT:
        _COLOUR_LUT[dev, depth] = _to_bytes(_levels_to_float(torch.arange(1 << depth, dtype=torch.float32, device=dev), depth)).contiguous()
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()         # later calls may read it from any stream
    return _COLOUR_LUT[dev, depth]


class _Frames:
    """What ``YUVFrames``, ``RawFrames`` and the packed frames share: N frames of one view, sliced by frame range only and moved as a whole.  A subclass has ``n``,
    ``_tensors()`` (its planes; the first names the device), ``_like(*planes)`` and ``_moved(device)`` -- and for its front door ``_entry`` (the
    entry point's name), ``view_struct()``, ``_structs()`` (the structs that follow the two views), ``table(device)`` (the level table of the launch),
    ``levels_to_float(levels)`` and ``format_fault(other)`` (why ``other`` is no second view beside these frames, or None)."""

    def __len__(self) -> int:
        return self.n

    @property
    def device(self) -> torch.device:
        return self._tensors()[0].device

    def __getitem__(self, frames: slice):
        if not isinstance(frames, slice):
            raise TypeError(f"{type(self).__name__}: index with a slice of frames")
        return self._like(*(t[frames] for t in self._tensors()))

    def to(self, device):
        """These frames on ``device`` ("cuda" without an index: the current device), dense; frames already there are returned as they are."""
        device = _moved_to(device)
        return self if self.device == device else self._moved(device)


class _StereoVideo:
    """What ``YUVStereoVideo``, ``RawStereoVideo`` and their packed twins share: two frame objects of class ``_views`` with one size, frame count and device (a fault
    there is reported as "both views need ``_one``") and one format -- ``left.format_fault(right)``: what differs, or None.  ``len()``, slicing
    by frame range, ``to(device)``."""
    _views: type
    _one = "one device"

    def __init__(self, left, right):
        name = type(self).__name__
        if not isinstance(left, self._views) or not isinstance(right, self._views):
            raise TypeError(f"{name}: two {self._views.__name__} expected")
        if (left.n, left.height, left.width) != (right.n, right.height, right.width):
            raise ValueError(f"{name}: the views differ: {(left.n, left.height, left.width)} and {(right.n, right.height, right.width)}")
        fault = f"both views need {self._one}" if left.device != right.device else left.format_fault(right)
        if fault:
            raise ValueError(f"{name}: {fault}")
        self.left, self.right = left, right
        self.depth = left.depth
        self.height, self.width = left.height, left.width

    def __len__(self) -> int:
        return self.left.n

    def __getitem__(self, frames: slice):
        return type(self)(self.left[frames], self.right[frames])

    def to(self, device):
        """The selected frames on ``device``: each view's own bytes are copied (``YUVFrames.to`` / ``RawFrames.to``)."""
        return type(self)(self.left.to(device), self.right.to(device))


_YUV_STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}       # (Kr, Kb)
_CHROMA = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}                      # (sub_x, sub_y): log2 of the chroma subsampling


def yuv_matrix(standard: str = "bt709", full_range: bool = False, shift: int = 14, depth: int = 8) -> L.YUVMatrix:
    """The fixed-point YCbCr -> RGB conversion ppms_video_ingest_yuv420 / ppms_video_ingest_yuv apply (include/ppms.h), as their
    ``ppms_yuv_matrix``: Python ``round()`` of the double-precision coefficients times 2^shift.  Limited range at depth 8: Y in [16, 235], chroma
    in [16, 240]; at depth d those bounds times 2^(d - 8), stretched to [0, 2^d - 1].  Not covered: "bt2020" (refused)."""
    if standard not in _YUV_STANDARDS:
        raise ValueError(f"yuv_matrix: standard {standard!r}; one of {sorted(_YUV_STANDARDS)}")
    depth = _check_depth("yuv_matrix", depth)
    top_shift = 20 if depth == 8 else 26 - depth
    if not 8 <= shift <= top_shift:
        raise ValueError(f"yuv_matrix: shift = {shift} must lie in [8, {top_shift}]")
    kr, kb = _YUV_STANDARDS[standard]
    kg = 1.0 - kr - kb
    maxv, up = (1 << depth) - 1, depth - 8
    sy, sc = (1.0, 1.0) if full_range else (maxv / (219 << up), maxv / (224 << up))
    one = float(1 << shift)
    return L.YUVMatrix(y_off=0 if full_range else 16 << up, cy=round(sy * one), crv=round(sc * 2.0 * (1.0 - kr) * one),
                       cgu=round(sc * 2.0 * kb * (1.0 - kb) / kg * one), cgv=round(sc * 2.0 * kr * (1.0 - kr) / kg * one),
                       cbu=round(sc * 2.0 * (1.0 - kb) * one), shift=shift, reserved=0)


class _YUVColour:
    """What ``YUVFrames`` and ``PackedYUVFrames`` share: ``standard``, ``full_range`` and ``depth`` choose the matrix, the level table is ``level_lut``'s
    of that depth, and two views need one standard and one range."""

    def matrix(self) -> L.YUVMatrix:
        return yuv_matrix(self.standard, self.full_range, depth=self.depth)

    def table(self, device) -> torch.Tensor:
        return level_lut(device, self.depth)

    def colour_table(self, device) -> torch.Tensor:
        return colour_lut(device, self.depth)

    def levels_to_float(self, levels: torch.Tensor) -> torch.Tensor:
        return _levels_to_float(levels, self.depth)

    def _colour_fault(self, other) -> Optional[str]:
        if (self.standard, self.full_range) != (other.standard, other.full_range):
            return "both views need one standard, one range and one device"
        return None


class YUVFrames(_YUVColour, _Frames):
    """One view's N decoded YUV frames, as a decoder leaves them: ``y`` (N, H0, W0), ``u`` / ``v`` (N, ceil(H0 / 2), ceil(W0 / 2)) for
    ``chroma="420"`` (the default), (N, H0, ceil(W0 / 2)) for "422", (N, H0, W0) for "444".  ``depth=8`` (the default): uint8 planes; ``depth`` 10 or 12:
    ``torch.uint16`` planes whose words hold the sample at the top (``align="msb"``: P010 / P012 / P210; the low bits are dropped whatever they hold)
    or at the bottom (``align="lsb"``: yuv420p10le ...; the high bits are masked).  Each may be a strided VIEW of a decoder surface -- a pitched plane, the two halves of an interleaved
    UV plane (``nv12``), one half of a frame that packs both views (``split_side_by_side`` / ``split_top_bottom``): the class reads
    ``data_ptr()`` and ``stride()`` and never copies.  ``y`` needs last-dimension stride 1; ``u`` and ``v`` equal strides with
    last-dimension stride 1 (planar: I420 / yuv420p) or 2 (interleaved: NV12); anything else raises ValueError.  Strides are read in elements
    and kept in BYTES (``pitch_y`` ..., what ``ppms_yuv_view`` holds).  Luma pixel (y, x) takes chroma sample (y >> sub_y, x >> sub_x), nearest;
    ``standard`` ("bt709" / "bt601") and ``full_range`` choose ``yuv_matrix``; ``to_rgb`` is the definition of the RGB levels (``to_rgb_u8``: of the
    bytes at depth 8).  Packed 4:2:2 (YUYV / Y210 / v210): ``PackedYUVFrames``.  Not covered: interpolated chroma siting, 16-bit depth, BT.2020
    and HDR transfer functions, b > 1."""

    def __init__(self, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, standard: str = "bt709", full_range: bool = False, depth: int = 8,
                 align: str = "msb", chroma: str = "420"):
        depth = _check_depth("YUVFrames", depth)
        dtype, es = (torch.uint8, 1) if depth == 8 else (torch.uint16, 2)
        lsb = _sample_lsb("YUVFrames", align, depth, es == 2)
        if chroma not in _CHROMA:
            raise ValueError(f"YUVFrames: chroma {chroma!r}; one of {sorted(_CHROMA)}")
        for name, t in (("y", y), ("u", u), ("v", v)):
            _check_plane("YUVFrames", name, t, dtype, depth=depth)
        n, h0, w0 = y.shape
        sub_x, sub_y = _CHROMA[chroma]
        hc, wc = (h0 + (1 << sub_y) - 1) >> sub_y, (w0 + (1 << sub_x) - 1) >> sub_x
        if n < 1 or h0 < 1 or w0 < 1:
            raise ValueError(f"YUVFrames: empty y plane {tuple(y.shape)}")
        if tuple(u.shape) != (n, hc, wc) or tuple(v.shape) != (n, hc, wc):
            raise ValueError(f"YUVFrames: y {tuple(y.shape)} needs u and v of {(n, hc, wc)}, got {tuple(u.shape)} and {tuple(v.shape)}")
        if u.device != y.device or v.device != y.device:
            raise ValueError("YUVFrames: y, u and v must be on one device")
        if w0 > 1 and y.stride(2) != 1:
            raise ValueError(f"YUVFrames: y has last-dimension stride {y.stride(2)}; luma samples must be adjacent bytes")
        step = u.stride(2) if wc > 1 else 1                                # (a one-column chroma plane never takes a step)
        if u.stride() != v.stride():
            raise ValueError(f"YUVFrames: u and v must have equal strides, got {u.stride()} and {v.stride()}")
        if step not in (1, 2):
            raise ValueError(f"YUVFrames: chroma last-dimension stride {step}; 1 (planar) or 2 (interleaved) expected")
        if es == 2 and any(t.data_ptr() % 2 for t in (y, u, v)):
            raise ValueError("YUVFrames: 16-bit planes must start at even addresses")
        luma, chroma_strides = _strides(y, w0), _strides(u, step * (wc - 1) + 1)      # (elements here, bytes below)
        if luma is None or chroma_strides is None:
            raise ValueError(f"YUVFrames: rows or frames overlap (y strides {y.stride()}, chroma strides {u.stride()})")
        (self.pitch_y, self.frame_stride_y), (self.pitch_c, self.frame_stride_c) = ((p * es, f * es) for p, f in (luma, chroma_strides))
        self.step_c = step * es
        yuv_matrix(standard)                                               # (refuses an unknown standard here)
        self.y, self.u, self.v, self.standard, self.full_range = y, u, v, standard, bool(full_range)
        self.n, self.height, self.width = n, h0, w0
        self.depth, self.align, self.chroma, self.sample_bytes = depth, align, chroma, es
        self.sub_x, self.sub_y, self.lsb = sub_x, sub_y, lsb
        # the door: 8-bit 4:2:0 has an entry point of its own, which takes no format (it writes ppms_video_ingest_yuv's bits a tenth sooner)
        self._entry = "ppms_video_ingest_yuv420" if (depth, chroma) == (8, "420") else "ppms_video_ingest_yuv"

    @classmethod
    def nv12(cls, y: torch.Tensor, uv: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """NV12: ``uv`` uint8 (N, ceil(H0 / 2), ceil(W0 / 2), 2), U first -- a hardware decoder's surface."""
        if not torch.is_tensor(uv) or uv.dim() != 4 or uv.shape[-1] != 2:
            raise ValueError("YUVFrames.nv12: uv must be (N, rows, columns, 2)")
        return cls(y, uv[..., 0], uv[..., 1], standard, full_range)

    @classmethod
    def nv16(cls, y: torch.Tensor, uv: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """NV16: 8-bit 4:2:2, ``uv`` uint8 (N, H0, ceil(W0 / 2), 2), U first -- what an MJPEG decoder leaves."""
        return cls._interleaved("nv16", y, uv, standard, full_range, 8, "422")

    @classmethod
    def p010(cls, y: torch.Tensor, uv: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """P010: 10-bit 4:2:0 in 16-bit words, the sample in the top 10 bits; ``uv`` uint16 (N, ceil(H0 / 2), ceil(W0 / 2), 2), U first -- a
        hardware decoder's HEVC / AV1 Main10 surface."""
        return cls._interleaved("p010", y, uv, standard, full_range, 10, "420")

    @classmethod
    def p210(cls, y: torch.Tensor, uv: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """P210: P010's words with 4:2:2 chroma; ``uv`` uint16 (N, H0, ceil(W0 / 2), 2)."""
        return cls._interleaved("p210", y, uv, standard, full_range, 10, "422")

    @classmethod
    def _interleaved(cls, name, y, uv, standard, full_range, depth, chroma) -> "YUVFrames":
        if not torch.is_tensor(uv) or uv.dim() != 4 or uv.shape[-1] != 2:
            raise ValueError(f"YUVFrames.{name}: uv must be (N, rows, columns, 2)")
        return cls(y, uv[..., 0], uv[..., 1], standard, full_range, depth, "msb", chroma)

    @classmethod
    def planar(cls, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, chroma: str = "420", align: str = "lsb",
               standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """Three planes of any covered depth and subsampling -- a software decoder's yuv420p10le / yuv422p10le / yuv444p12le / yuv422p / yuv444p."""
        return cls(y, u, v, standard, full_range, depth, align, chroma)

    @classmethod
    def i420(cls, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """I420 / yuv420p: three planes -- a software decoder's frame."""
        return cls(y, u, v, standard, full_range)

    def _tensors(self):
        return self.y, self.u, self.v

    def _like(self, y, u, v) -> "YUVFrames":
        return YUVFrames(y, u, v, self.standard, self.full_range, self.depth, self.align, self.chroma)

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side; views, no copy.  The packed width must be even --
        and with subsampled chroma each half's too, or the right half's chroma would start between two samples."""
        w = self.width
        if w % 2 or (w // 2) % (1 << self.sub_x):
            raise ValueError(f"YUVFrames.split_side_by_side: a packed width of {w} does not split into two views with whole chroma samples")
        h, q = w // 2, (w // 2) >> self.sub_x
        return (self._like(self.y[:, :, :h], self.u[:, :, :q], self.v[:, :, :q]), self._like(self.y[:, :, h:], self.u[:, :, q:], self.v[:, :, q:]))

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy (even halves, as above)."""
        ht = self.height
        if ht % 2 or (ht // 2) % (1 << self.sub_y):
            raise ValueError(f"YUVFrames.split_top_bottom: a packed height of {ht} does not split into two views with whole chroma rows")
        h, q = ht // 2, (ht // 2) >> self.sub_y
        return (self._like(self.y[:, :h], self.u[:, :q], self.v[:, :q]), self._like(self.y[:, h:], self.u[:, q:], self.v[:, q:]))

    def _moved(self, device) -> "YUVFrames":
        """``to``: the planes' own bytes are copied (8-bit 4:2:0: 1.5 per pixel, 4:2:2: 2, 4:4:4: 3; twice that for 16-bit samples; an
        interleaved UV plane as one block) into dense planes."""
        y = self.y.to(device)
        if self.step_c == 2 * self.sample_bytes and self.v.data_ptr() == self.u.data_ptr() + self.sample_bytes:
            uv = torch.as_strided(self.u, (*self.u.shape, 2), (*self.u.stride(), 1)).to(device)
            return self._like(y, uv[..., 0], uv[..., 1])
        return self._like(y, self.u.to(device), self.v.to(device))

    def format_fault(self, other: "YUVFrames") -> Optional[str]:
        fault = self._colour_fault(other)
        if fault is None and (self.depth, self.lsb, self.chroma) != (other.depth, other.lsb, other.chroma):
            fault = f"the views differ in depth, alignment or chroma: {(self.depth, self.align, self.chroma)} and {(other.depth, other.align, other.chroma)}"
        return fault

    def format_struct(self) -> L.YUVFormat:
        """The ``ppms_yuv_format`` of these frames."""
        return L.YUVFormat(self.sample_bytes, self.depth, self.lsb, self.sub_x, self.sub_y, (0, 0, 0))

    def _structs(self):
        return (self.matrix(),) if self._entry.endswith("420") else (self.matrix(), self.format_struct())

    def view_struct(self) -> L.YUVView:
        """The ``ppms_yuv_view`` of these frames."""
        return L.YUVView(self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), self.frame_stride_y, self.frame_stride_c, self.pitch_y, self.pitch_c,
                         self.step_c, 0)

    def to_rgb(self) -> torch.Tensor:
        """(N, 3, H0, W0) on the same device, uint8 at depth 8 and int16 levels in [0, 2^depth - 1] otherwise: the conversion of include/ppms.h in
        torch integer ops -- what the feature means by the RGB levels of these frames (the kernels' operands are ppms_video_ingest_u8's on them,
        with the table of that depth), and the path where the kernels cannot be used."""
        m = self.matrix()
        top = (1 << self.depth) - 1
        rows = torch.arange(self.height, device=self.device) >> self.sub_y
        cols = torch.arange(self.width, device=self.device) >> self.sub_x
        sample = lambda t: (t.to(torch.int32) >> self.lsb) & top
        d = sample(self.y) - m.y_off
        e, f = (sample(c)[:, rows][:, :, cols] - (1 << (self.depth - 1)) for c in (self.u, self.v))
        r = 1 << (m.shift - 1)
        rgb = torch.stack([m.cy * d + m.crv * f + r, m.cy * d - m.cgu * e - m.cgv * f + r, m.cy * d + m.cbu * e + r], dim=1)
        return (rgb >> m.shift).clamp_(0, top).to(torch.uint8 if self.depth == 8 else torch.int16)

    def to_rgb_u8(self) -> torch.Tensor:
        """``to_rgb`` of 8-bit frames: uint8 (N, 3, H0, W0).  Deep frames have no RGB bytes (ValueError): their levels are ``to_rgb``'s."""
        if self.depth != 8:
            raise ValueError(f"YUVFrames.to_rgb_u8: the frames hold {self.depth}-bit samples; to_rgb() gives their levels, to_float() the float video")
        return self.to_rgb()

    def to_float(self) -> torch.Tensor:
        """float32 (N, 3, H0, W0) in [0, 255]: ``levels.float() * (255.0 / (2^depth - 1))`` -- the video the reference would be given."""
        return _levels_to_float(self.to_rgb(), self.depth)


class YUVStereoVideo(_StereoVideo):
    """Both views of a decoded YUV video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor:
    two ``YUVFrames`` of one size, frame count, device, colour description and sample format (depth, alignment, chroma subsampling).  ``len()``,
    slicing by frame range, ``to(device)`` (8-bit 4:2:0: 1.5 bytes per pixel and view; P010: 3)."""
    _views, _one = YUVFrames, "one standard, one range and one device"


_RAW_PATTERNS = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3, "mono": 4}           # ppms_raw_format.pattern
_RAW_SHIFT = 10                                                                    # the white-balance gains' fixed point


class _RawFormat:
    """What ``RawFrames`` and ``PackedRawFrames`` say about the sensor, checked once: ``pattern``, ``depth``, ``black``, ``gains`` (``gain_q``:
    quantised), ``tone`` -- and the tone curve and the ingest table per device, each made once.  Every slice, half and copy of the frames holds
    the same object.  (The messages name ``RawFrames``, whose arguments these are, for the packed frames too.)"""

    def __init__(self, pattern: str, depth: int, black: int, gains, tone: Optional[torch.Tensor]):
        if pattern not in _RAW_PATTERNS:
            raise ValueError(f"RawFrames: pattern {pattern!r}; one of {sorted(_RAW_PATTERNS)}")
        if not (isinstance(black, int) and 0 <= black < (1 << depth)):
            raise ValueError(f"RawFrames: black = {black!r} must be an integer level in [0, {(1 << depth) - 1}]")
        try:
            gains = tuple(float(g) for g in gains)
        except (TypeError, ValueError):
            raise ValueError(f"RawFrames: gains = {gains!r} must be three numbers (R, G, B)") from None
        if len(gains) != 3 or not all(0.0 <= g < 16.0 and 0 <= round(g * (1 << _RAW_SHIFT)) < (16 << _RAW_SHIFT) for g in gains):
            raise ValueError(f"RawFrames: gains = {gains!r} must be three numbers (R, G, B) in [0, 16)")
        if tone is not None:
            if not torch.is_tensor(tone) or not tone.is_floating_point() or tuple(tone.shape) != (1 << depth,):
                raise ValueError(f"RawFrames: tone must be a floating-point tensor of {1 << depth} values, one per level of {depth} bits")
            tone = tone.detach().to(torch.float32)
            if not bool(((tone >= 0.0) & (tone <= 255.0)).all()):
                raise ValueError("RawFrames: tone holds values outside [0, 255]")
        self.pattern, self.depth, self.black, self.gains, self.tone = pattern, depth, black, gains, tone
        self.gain_q = tuple(round(g * (1 << _RAW_SHIFT)) for g in gains)
        self._tone_on: Dict[torch.device, torch.Tensor] = {}
        self._table_on: Dict[torch.device, torch.Tensor] = {}
        self._colour_on: Dict[torch.device, torch.Tensor] = {}

    def same_format(self, other: "_RawFormat") -> bool:
        """One pattern, depth, black level, white balance and tone curve."""
        if (self.pattern, self.depth, self.black, self.gain_q) != (other.pattern, other.depth, other.black, other.gain_q):
            return False
        if self.tone is None or other.tone is None or self.tone is other.tone:
            return self.tone is other.tone
        return torch.equal(self.tone.cpu(), other.tone.cpu())

    def tone_on(self, device) -> Optional[torch.Tensor]:
        """``tone`` on ``device`` (None stays None); copied there once."""
        if self.tone is None:
            return None
        device = torch.device(device)
        if device not in self._tone_on:
            self._tone_on[device] = self.tone.to(device).contiguous()
        return self._tone_on[device]

    def levels_to_float(self, levels: torch.Tensor) -> torch.Tensor:
        """RGB levels (``to_rgb``'s, or their remap) -> the float32 video in [0, 255] they stand for: ``tone[level]``, or without a tone curve
        ``level * (255.0 / (2^depth - 1))``."""
        tone = self.tone_on(levels.device)
        return _levels_to_float(levels, self.depth) if tone is None else tone[levels.long()]

    def table(self, device) -> torch.Tensor:
        """fp32 [2^depth] on ``device``: the normalised value of every level, what the ingest kernel looks up.  Without a tone curve
        ``level_lut``'s tensor; with one ``2 * (tone / 255.0) - 1.0`` computed ON THE DEVICE, ``forward``'s own expression on ``to_float``'s
        values -- for ``byte_lut``'s reason.  Built once per device and kept with the frames (the host waits for it once)."""
        if self.tone is None:
            return level_lut(device, self.depth)
        dev = torch.device("cuda", _cuda_index(device))
        if dev not in self._table_on:
            self._table_on[dev] = (2 * (self.tone_on(dev) / 255.0) - 1.0).contiguous()
            torch.cuda.current_stream(dev).synchronize()         # later calls may read it from any stream
        return self._table_on[dev]

    def colour_table(self, device) -> torch.Tensor:
        """uint8 [2^depth] on ``device`` (a GPU, or the host): the colour byte of every level, what the colour kernel looks up.  Without a tone
        curve ``colour_lut``'s tensor; with one clamp(rint(tone), 0, 255).  Built once per device and kept with the frames."""
        if self.tone is None:
            return colour_lut(device, self.depth)
        dev = _moved_to(device)
        if dev not in self._colour_on:
            self._colour_on[dev] = _to_bytes(self.tone_on(dev)).contiguous()
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()     # later calls may read it from any stream
        return self._colour_on[dev]


class _RawSensor:
    """What ``RawFrames`` and ``PackedRawFrames`` share: one ``_RawFormat``, whose ``pattern``, ``black``, ``gains``, ``gain_q`` and ``tone`` are
    the frames' own attributes and whose tone curve and table are the frames'."""

    def _describe(self, fmt: _RawFormat) -> None:
        self._format = fmt
        self.pattern, self.black, self.gains, self.gain_q, self.tone = fmt.pattern, fmt.black, fmt.gains, fmt.gain_q, fmt.tone

    def tone_on(self, device) -> Optional[torch.Tensor]:
        return self._format.tone_on(device)

    def levels_to_float(self, levels: torch.Tensor) -> torch.Tensor:
        return self._format.levels_to_float(levels)

    def table(self, device) -> torch.Tensor:
        """The frames' own level table on ``device`` (``_RawFormat.table``), built once and shared by every slice, half and copy."""
        return self._format.table(device)

    def colour_table(self, device) -> torch.Tensor:
        """The frames' own colour-byte table on ``device`` (``_RawFormat.colour_table``), shared likewise."""
        return self._format.colour_table(device)


class RawFrames(_RawSensor, _Frames):
    """One view's N raw sensor frames, as a camera driver leaves them: ``data`` (N, H0, W0), one sample per pixel under the colour-filter mosaic
    ``pattern`` ("rggb" / "bggr" / "grbg" / "gbrg": the 2 x 2 tile at the frame's origin, row-major -- BayerRG8, BayerGB10 ...) or "mono"
    (Mono8 / Mono10 / Mono12).  ``depth=8``: a uint8 plane; ``depth`` 10 or 12: a ``torch.uint16`` plane whose words hold the sample at the bottom
    (``align="lsb"``, the default: the high bits are masked) or at the top (``align="msb"``: the low bits are dropped whatever they hold).  ``data`` may
    be a strided VIEW of a driver's buffer -- pitched rows, one half of a frame that packs both views (``split_side_by_side`` /
    ``split_top_bottom``): the class reads ``data_ptr()`` and ``stride()`` and never copies; last-dimension stride 1, rows and frames that do not
    overlap, anything else raises ValueError.  Strides are kept in BYTES (what ``ppms_raw_view`` holds).  ``black`` is the sensor's black level,
    ``gains`` the white balance for (R, G, B), quantised with ``round(g * 1024)``; ``to_rgb`` is the definition of the RGB levels (bilinear
    demosaic with reflected borders, include/ppms.h).  ``tone``: None -- a level stands for ``level * 255 / (2^depth - 1)`` -- or a float tensor of
    2^depth values in [0, 255], the value each level stands for: where the gamma / sRGB encoding of linear sensor data goes, at no cost (the
    kernel looks every level up in a table anyway).  Packed 10p / 12p transport formats: ``PackedRawFrames``.  Not covered: 14- and 16-bit sensors,
    demosaicing better than bilinear, colour-correction matrices, lens shading and defect pixels, per-view differing patterns, b > 1."""

    _entry = "ppms_video_ingest_raw"

    def __init__(self, data: torch.Tensor, pattern: str = "rggb", depth: int = 8, align: str = "lsb", black: int = 0, gains=(1.0, 1.0, 1.0),
                 tone: Optional[torch.Tensor] = None, _format: Optional[_RawFormat] = None):
        depth = _check_depth("RawFrames", depth)
        # (a slice, half or copy passes its frames' own format on: checked once, one tone curve and one table per device for all of them)
        self._describe(_RawFormat(pattern, depth, black, gains, tone) if _format is None else _format)
        dtype, es = (torch.uint8, 1) if depth == 8 else (torch.uint16, 2)
        lsb = _sample_lsb("RawFrames", align, depth, es == 2)
        _check_plane("RawFrames", "data", data, dtype, depth=depth)
        n, h0, w0 = data.shape
        if n < 1 or h0 < 1 or w0 < 1:
            raise ValueError(f"RawFrames: empty plane {tuple(data.shape)}")
        if self.pattern != "mono" and (h0 < 2 or w0 < 2):
            raise ValueError(f"RawFrames: a colour pattern needs frames of at least 2 x 2, got {h0} x {w0}")
        if w0 > 1 and data.stride(2) != 1:
            raise ValueError(f"RawFrames: data has last-dimension stride {data.stride(2)}; samples must be adjacent")
        if es == 2 and data.data_ptr() % 2:
            raise ValueError("RawFrames: a 16-bit plane must start at an even address")
        strides = _strides(data, w0)                                       # (elements here, bytes below)
        if strides is None:
            raise ValueError(f"RawFrames: rows or frames overlap (strides {data.stride()})")
        self.data, self.depth, self.align, self.lsb = data, depth, align, lsb
        self.n, self.height, self.width, self.sample_bytes = n, h0, w0, es
        self.pitch, self.frame_stride = strides[0] * es, strides[1] * es

    def _tensors(self):
        return (self.data,)

    def _like(self, data) -> "RawFrames":
        return RawFrames(data, depth=self.depth, align=self.align, _format=self._format)

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side; views, no copy.  The packed width must be even -- and with a
        colour pattern each half's too: a right half that starts on an odd column has another pattern than the left one."""
        w = self.width
        if w % 2 or (self.pattern != "mono" and (w // 2) % 2):
            raise ValueError(f"RawFrames.split_side_by_side: a packed width of {w} does not split into two views of one {self.pattern} pattern")
        return self._like(self.data[:, :, :w // 2]), self._like(self.data[:, :, w // 2:])

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy (even halves, as above)."""
        h = self.height
        if h % 2 or (self.pattern != "mono" and (h // 2) % 2):
            raise ValueError(f"RawFrames.split_top_bottom: a packed height of {h} does not split into two views of one {self.pattern} pattern")
        return self._like(self.data[:, :h // 2]), self._like(self.data[:, h // 2:])

    def _moved(self, device) -> "RawFrames":
        """``to``: the samples' own bytes are copied (1 per pixel, 2 for 16-bit words) into a dense plane."""
        return self._like(self.data.to(device))

    def same_format(self, other: "RawFrames") -> bool:
        """Both hold one kind of sample, under one pattern, with one black level, white balance and tone curve."""
        return self.lsb == other.lsb and self._format.same_format(other._format)

    def format_fault(self, other: "RawFrames") -> Optional[str]:
        if self.same_format(other):
            return None
        return ("the views differ in pattern, depth, alignment, black level, gains or tone curve: "
                f"{(self.pattern, self.depth, self.align, self.black, self.gains)} and {(other.pattern, other.depth, other.align, other.black, other.gains)}")

    def format_struct(self) -> L.RawFormat:
        """The ``ppms_raw_format`` of these frames."""
        return L.RawFormat(self.sample_bytes, self.depth, self.lsb, _RAW_PATTERNS[self.pattern], self.black, self.gain_q, _RAW_SHIFT, (0, 0, 0))

    def _structs(self):
        return (self.format_struct(),)

    def view_struct(self) -> L.RawView:
        """The ``ppms_raw_view`` of these frames."""
        return L.RawView(self.data.data_ptr(), self.frame_stride, self.pitch, 0)

    def to_rgb(self) -> torch.Tensor:
        """(N, 3, H0, W0) on the same device, uint8 at depth 8 and int16 levels in [0, 2^depth - 1] otherwise: the demosaic, black level and white
        balance of include/ppms.h in torch integer ops -- what the feature means by the RGB levels of these frames (the kernels' operands are
        ppms_video_ingest_u8's on them, with ``table``), and the path where the kernels cannot be used."""
        top, h, w, dev = (1 << self.depth) - 1, self.height, self.width, self.device
        s = (self.data.to(torch.int32) >> self.lsb) & top
        if self.pattern == "mono":
            v = torch.stack([s, s, s], dim=1)
        else:
            # one sample of margin all round, reflected without repeating the edge: row -1 is row 1, row h is row h - 2
            ri = torch.tensor([1, *range(h), h - 2], device=dev)
            ci = torch.tensor([1, *range(w), w - 2], device=dev)
            p = s[:, ri][:, :, ci]
            at = lambda dy, dx: p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            hor, ver = (at(0, -1) + at(0, 1) + 1) >> 1, (at(-1, 0) + at(1, 0) + 1) >> 1
            cross = (at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1) + 2) >> 2
            diag = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2
            code = _RAW_PATTERNS[self.pattern]
            py, px = (torch.arange(h, device=dev) & 1)[:, None], (torch.arange(w, device=dev) & 1)[None, :]
            green = ((px ^ py ^ (code >> 1)) == 1).expand(h, w)
            red_row = ((py ^ (code & 1)) == 0).expand(h, w)               # rows whose non-green sites are red
            v = torch.stack([torch.where(green, torch.where(red_row, hor, ver), torch.where(red_row, s, diag)),
                             torch.where(green, s, cross),
                             torch.where(green, torch.where(red_row, ver, hor), torch.where(red_row, diag, s))], dim=1)
        gain = torch.tensor(self.gain_q, dtype=torch.int32, device=dev).reshape(1, 3, 1, 1)
        levels = ((v - self.black) * gain + (1 << (_RAW_SHIFT - 1))) >> _RAW_SHIFT
        return levels.clamp_(0, top).to(torch.uint8 if self.depth == 8 else torch.int16)

    def to_float(self) -> torch.Tensor:
        """float32 (N, 3, H0, W0) in [0, 255]: the video the reference would be given."""
        return self.levels_to_float(self.to_rgb())


class RawStereoVideo(_StereoVideo):
    """Both views of a raw sensor video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor: two
    ``RawFrames`` of one size, frame count, device, pattern, sample format (depth, alignment), black level, white balance and tone curve.
    ``len()``, slicing by frame range, ``to(device)`` (1 byte per pixel and view; 2 for 10- and 12-bit samples)."""
    _views = RawFrames


class _PackedFrames(_Frames):
    """What ``PackedYUVFrames``, ``PackedRawFrames`` and ``PackedRGBFrames`` share: ``data`` (N, H0, row elements) is the driver's own buffer -- a pitched SURFACE whose
    rows hold whole groups of ``_group`` = (pixels, elements) -- and the view is its columns [x0, x0 + width): nothing is copied, and the two halves
    of a side-by-side frame are one surface with two ``x0``.  A subclass has ``_name``, ``_group``, ``_align`` (bytes: what pointer and strides must
    be multiples of), ``_row_elements(P)`` (the elements of a row of P columns) and ``_with(data, x0, width)``."""

    def _surface(self, data: torch.Tensor, width, x0, dtype, pair: bool) -> None:
        name = self._name
        _check_plane(name, "data", data, dtype, "(N, rows, row elements)")
        if not (isinstance(width, int) and isinstance(x0, int) and width >= 1 and x0 >= 0 and x0 + width <= 65536):
            raise ValueError(f"{name}: width = {width!r}, x0 = {x0!r} must be integers with width >= 1, x0 >= 0 and x0 + width <= 65536")
        if pair and x0 % 2:
            raise ValueError(f"{name}: x0 = {x0} must be even: a chroma pair may not be split")
        n, h0, row = data.shape
        need = self._row_elements(x0 + width)
        if n < 1 or h0 < 1:
            raise ValueError(f"{name}: empty surface {tuple(data.shape)}")
        if row < need:
            raise ValueError(f"{name}: rows of {row} elements do not hold columns [{x0}, {x0 + width}): {need} are needed")
        if row > 1 and data.stride(2) != 1:
            raise ValueError(f"{name}: data has last-dimension stride {data.stride(2)}; a row's elements must be adjacent")
        es = data.element_size()
        strides = _strides(data, need)                                     # (elements here, bytes below)
        if strides is None:
            raise ValueError(f"{name}: rows or frames overlap (strides {data.stride()})")
        pitch, frame = strides
        if data.data_ptr() % self._align or (pitch * es) % self._align or (frame * es) % self._align:
            raise ValueError(f"{name}: the surface's address, pitch and frame stride must be multiples of {self._align} bytes")
        self.data, self.x0, self.n, self.height, self.width = data, x0, n, h0, width
        self.pitch, self.frame_stride = pitch * es, frame * es

    def _tensors(self):
        return (self.data,)

    def _like(self, data):
        return self._with(data, self.x0, self.width)

    def view_struct(self) -> L.PackedView:
        """The ``ppms_packed_view`` of these frames."""
        return L.PackedView(self.data.data_ptr(), self.frame_stride, self.pitch, self.x0)

    def _half(self, what: str, size: int, even_half: bool, views: str) -> int:
        if size % 2 or (even_half and (size // 2) % 2):
            raise ValueError(f"{self._name}.{what}: a packed {'width' if what == 'split_side_by_side' else 'height'} of {size} does not split into two {views}")
        return size // 2

    def _moved(self, device):
        """``to``: the packed bytes of the view's own groups are copied -- from the group that holds column x0 to the end of the row of column
        x0 + width - 1 -- into a dense surface; ``x0`` becomes the column inside that first group."""
        pixels, elements = self._group
        g = self.x0 // pixels
        return self._with(self.data[:, :, g * elements:self._row_elements(self.x0 + self.width)].to(device), self.x0 - g * pixels, self.width)

    def to_rgb(self) -> torch.Tensor:
        """``unpack().to_rgb()``: (N, 3, H0, W0) RGB levels, uint8 at depth 8 and int16 otherwise."""
        return self.unpack().to_rgb()

    def to_float(self) -> torch.Tensor:
        """``unpack().to_float()``: float32 (N, 3, H0, W0) in [0, 255] -- the video the reference would be given."""
        return self.unpack().to_float()


_PACKED_YUV = {"yuyv": (0, 8, 0), "uyvy": (0, 8, 1), "yvyu": (0, 8, 2), "vyuy": (0, 8, 3),      # layout: (container, depth, order) of
               "y210": (1, 10, 0), "y212": (1, 12, 0), "v210": (2, 10, 1)}                      # ppms_yuv_packed_format


def _packed_yuv_row(container: int, p: int) -> int:
    """The elements (bytes; 16-bit words for container 1) of a packed 4:2:2 row of p columns: whole pairs, for v210 whole groups of 6 pixels."""
    return 16 * (-(-p // 6)) if container == 2 else 4 * (-(-p // 2))


def _packed_yuv_indices(order: int, x0: int, width: int, device):
    """The component indices of surface columns [x0, x0 + width) (x0 even): Y per pixel, U and V per pair (include/ppms.h)."""
    a = order & 1
    p = torch.arange(x0, x0 + width, device=device)
    j = torch.arange(x0 // 2, (x0 + width + 1) // 2, device=device)
    return 2 * p + a, 4 * j + (1 - a + (order & 2)), 4 * j + (3 - order)


class PackedYUVFrames(_YUVColour, _PackedFrames):
    """One view's N frames of packed 4:2:2 YUV, as a UVC camera or a capture card leaves them: ``data`` (N, H0, row elements) over the driver's own
    buffer, ``width`` pixels wide.  ``layout`` "yuyv" (YUY2) / "uyvy" / "yvyu" / "vyuy": uint8, 4 bytes per pixel pair in that order; "y210" /
    "y212": ``torch.uint16`` words in yuyv order holding 10 / 12 bits at the top (``align="msb"``, the default: Y210 / Y212; the low bits are
    dropped whatever they hold) or at the bottom (``align="lsb"``); "v210": uint8, 6 pixels in 16 bytes -- three 10-bit components per
    little-endian 32-bit word, Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5 (include/ppms.h is the definition; not compared with ffmpeg); its
    address, pitch and frame stride are multiples of 4.  A row holds whole pairs (v210: whole groups).  ``data`` may be a strided view; the class
    reads ``data_ptr()`` and ``stride()`` and never copies.  ``unpack`` is the definition of the samples, ``to_rgb`` / ``to_float`` those of the
    planar frames it returns (chroma from the pixel's own pair, nearest).  Not covered: Y216 and other 16-bit depths, 4:4:4 packed (v410, Y410,
    AYUV), big-endian containers, interpolated chroma siting, b > 1.  (Interleaved RGB: ``PackedRGBFrames``.)"""
    _name, _entry = "PackedYUVFrames", "ppms_video_ingest_yuv_packed"

    def __init__(self, data: torch.Tensor, width: int, layout: str = "yuyv", align: str = "msb", standard: str = "bt709", full_range: bool = False,
                 x0: int = 0):
        if layout not in _PACKED_YUV:
            raise ValueError(f"PackedYUVFrames: layout {layout!r}; one of {sorted(_PACKED_YUV)}")
        self.container, self.depth, self.order = _PACKED_YUV[layout]
        self.lsb = _sample_lsb("PackedYUVFrames", align, self.depth, self.container == 1)
        self._align = (1, 2, 4)[self.container]
        self._group = (6, 16) if self.container == 2 else (2, 4)
        self._surface(data, width, x0, torch.uint16 if self.container == 1 else torch.uint8, True)
        yuv_matrix(standard)                                               # (refuses an unknown standard here)
        self.layout, self.align, self.standard, self.full_range = layout, align, standard, bool(full_range)

    def _row_elements(self, p: int) -> int:
        return _packed_yuv_row(self.container, p)

    def _with(self, data, x0, width) -> "PackedYUVFrames":
        return PackedYUVFrames(data, width, self.layout, self.align, self.standard, self.full_range, x0)

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side -- the same surface with two ``x0``.  The packed width and
        each half must be even, or the right half would start inside a chroma pair."""
        h = self._half("split_side_by_side", self.width, True, "views with whole chroma pairs")
        return self._with(self.data, self.x0, h), self._with(self.data, self.x0 + h, h)

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy."""
        h = self._half("split_top_bottom", self.height, False, "views")
        return self._like(self.data[:, :h]), self._like(self.data[:, h:])

    def format_fault(self, other: "PackedYUVFrames") -> Optional[str]:
        fault = self._colour_fault(other)
        if fault is None and (self.layout, self.lsb) != (other.layout, other.lsb):
            fault = f"the views differ in layout or alignment: {(self.layout, self.align)} and {(other.layout, other.align)}"
        return fault

    def format_struct(self) -> L.YUVPackedFormat:
        """The ``ppms_yuv_packed_format`` of these frames."""
        return L.YUVPackedFormat(self.container, self.depth, self.lsb, self.order, (0, 0, 0, 0))

    def _structs(self):
        return self.matrix(), self.format_struct()

    def unpack(self) -> YUVFrames:
        """The ``YUVFrames.planar(..., chroma="422")`` holding the same samples (uint8, or uint16 with the bits at the bottom), in torch integer
        ops: the definition of the format on this side, and the path of encoder callables of the caller."""
        if self.container == 2:
            b = self.data.to(torch.int64).unflatten(2, (-1, 4))
            words = b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | b[..., 3] << 24
            component = lambda i: (words[:, :, i // 3] >> (10 * (i % 3))) & 1023
        else:
            component = lambda i: (self.data[:, :, i].to(torch.int32) >> self.lsb) & ((1 << self.depth) - 1)
        indices = _packed_yuv_indices(self.order, self.x0, self.width, self.device)
        y, u, v = (component(i).to(torch.uint8 if self.depth == 8 else torch.uint16) for i in indices)
        return YUVFrames.planar(y, u, v, self.depth, "422", "lsb", self.standard, self.full_range)

    @classmethod
    def pack(cls, frames: YUVFrames, layout: str = "yuyv", align: str = "msb") -> "PackedYUVFrames":
        """The inverse of ``unpack`` for simulators: 4:2:2 ``YUVFrames`` of the layout's depth -> dense packed rows (unused bits, and the second
        luma of an odd width's last pair, are 0)."""
        if not isinstance(frames, YUVFrames) or layout not in _PACKED_YUV or frames.chroma != "422" or frames.depth != _PACKED_YUV[layout][1]:
            raise ValueError(f"PackedYUVFrames.pack: 4:2:2 YUVFrames of the depth of layout {layout!r} (one of {sorted(_PACKED_YUV)}) expected")
        container, _, order = _PACKED_YUV[layout]
        top = (1 << frames.depth) - 1
        count = _packed_yuv_row(container, frames.width) * (3 if container == 2 else 4) // 4                  # components of a row (v210: 12 in 16 bytes)
        comp = torch.zeros((frames.n, frames.height, count), dtype=torch.int64, device=frames.device)
        for i, plane in zip(_packed_yuv_indices(order, 0, frames.width, frames.device), (frames.y, frames.u, frames.v)):
            comp[:, :, i] = (plane.to(torch.int64) >> frames.lsb) & top
        if container == 2:
            t = comp.unflatten(2, (-1, 3))
            words = t[..., 0] | t[..., 1] << 10 | t[..., 2] << 20
            data = torch.stack([(words >> s) & 255 for s in (0, 8, 16, 24)], dim=-1).flatten(2).to(torch.uint8)
        elif container == 1:
            data = (comp << (16 - frames.depth if align == "msb" else 0)).to(torch.int32).to(torch.uint16)
        else:
            data = comp.to(torch.uint8)
        return cls(data, frames.width, layout, align, frames.standard, frames.full_range)

    def to_rgb_u8(self) -> torch.Tensor:
        """``to_rgb`` of 8-bit layouts: uint8 (N, 3, H0, W0).  Deep layouts have no RGB bytes (ValueError)."""
        return self.unpack().to_rgb_u8()


class PackedYUVStereoVideo(_StereoVideo):
    """Both views of a packed 4:2:2 video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor: two
    ``PackedYUVFrames`` of one size, frame count, device, colour description, layout and alignment.  ``len()``, slicing by frame range,
    ``to(device)`` (the packed bytes: YUYV 2 per pixel and view, v210 2.67, Y210 4)."""
    _views, _one = PackedYUVFrames, "one standard, one range and one device"


_RAW_PACKINGS = {"mipi": 0, "pfnc": 1}                                             # ppms_raw_packed_format.packing


class PackedRawFrames(_RawSensor, _PackedFrames):
    """One view's N raw sensor frames in a packed transport format: ``data`` uint8 (N, H0, row bytes) over the driver's own buffer, ``width``
    pixels wide, ``depth`` 10 or 12 bits without padding.  ``packing="mipi"``: MIPI CSI-2 RAW10 / RAW12 as V4L2's SRGGB10P / SRGGB12P ... leave
    them -- the top 8 bits of 4 (2) pixels in 4 (2) bytes, their low bits together in a fifth (third); ``packing="pfnc"``: GenICam PFNC
    Mono10p / BayerRG12p ... -- an lsb-first bit stream, pixel p at bits [p depth, p depth + depth) of the row.  A row holds whole groups (pfnc:
    whole bytes).  ``pattern``, ``black``, ``gains`` and ``tone`` are ``RawFrames``'; ``x0`` may be any column, and the pattern is that of the
    view's own pixel (0, 0).  ``unpack`` is the definition of the samples, ``to_rgb`` / ``to_float`` those of the ``RawFrames`` it returns.  Not
    covered: 14-bit packed depths, packings whose rows are padded inside, patterns that differ between the views, b > 1."""
    _name, _align, _entry = "PackedRawFrames", 1, "ppms_video_ingest_raw_packed"

    def __init__(self, data: torch.Tensor, width: int, pattern: str = "rggb", depth: int = 10, packing: str = "mipi", black: int = 0,
                 gains=(1.0, 1.0, 1.0), tone: Optional[torch.Tensor] = None, x0: int = 0, _format: Optional[_RawFormat] = None):
        if depth not in (10, 12):
            raise ValueError(f"PackedRawFrames: depth = {depth!r}; 10 or 12")
        if packing not in _RAW_PACKINGS:
            raise ValueError(f"PackedRawFrames: packing {packing!r}; one of {sorted(_RAW_PACKINGS)}")
        self.depth, self.packing = depth, packing
        self._group = (4, 5) if depth == 10 else (2, 3)
        self._surface(data, width, x0, torch.uint8, False)
        # (a slice, half or copy passes its frames' own format on, as RawFrames does)
        self._describe(_RawFormat(pattern, depth, black, gains, tone) if _format is None else _format)
        if self.pattern != "mono" and (self.height < 2 or width < 2):
            raise ValueError(f"PackedRawFrames: a colour pattern needs frames of at least 2 x 2, got {self.height} x {width}")

    def _row_elements(self, p: int) -> int:
        return -(-p * self.depth // 8) if self.packing == "pfnc" else 5 * (-(-p // 4)) if self.depth == 10 else 3 * (-(-p // 2))

    def _with(self, data, x0, width) -> "PackedRawFrames":
        return PackedRawFrames(data, width, depth=self.depth, packing=self.packing, x0=x0, _format=self._format)

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side -- the same surface with two ``x0``.  The packed width must
        be even, and with a colour pattern each half's too (``RawFrames.split_side_by_side``)."""
        h = self._half("split_side_by_side", self.width, self.pattern != "mono", f"views of one {self.pattern} pattern")
        return self._with(self.data, self.x0, h), self._with(self.data, self.x0 + h, h)

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy (even halves, as above)."""
        h = self._half("split_top_bottom", self.height, self.pattern != "mono", f"views of one {self.pattern} pattern")
        return self._like(self.data[:, :h]), self._like(self.data[:, h:])

    def same_format(self, other: "PackedRawFrames") -> bool:
        """Both hold one packing of one depth, under one pattern, with one black level, white balance and tone curve."""
        return self.packing == other.packing and self._format.same_format(other._format)

    def format_fault(self, other: "PackedRawFrames") -> Optional[str]:
        if self.same_format(other):
            return None
        return ("the views differ in packing, depth, pattern, black level, gains or tone curve: "
                f"{(self.packing, self.depth, self.pattern, self.black, self.gains)} and {(other.packing, other.depth, other.pattern, other.black, other.gains)}")

    def format_struct(self) -> L.RawPackedFormat:
        """The ``ppms_raw_packed_format`` of these frames."""
        return L.RawPackedFormat(_RAW_PACKINGS[self.packing], self.depth, _RAW_PATTERNS[self.pattern], self.black, self.gain_q, _RAW_SHIFT, (0, 0, 0, 0))

    def _structs(self):
        return (self.format_struct(),)

    def unpack(self) -> RawFrames:
        """The ``RawFrames`` holding the same samples (uint16, bits at the bottom), in torch integer ops: the definition of the format on this
        side, and the path of encoder callables of the caller."""
        row = self.data.to(torch.int32)
        p = torch.arange(self.x0, self.x0 + self.width, device=self.device)
        if self.packing == "pfnc":
            bit = p * self.depth
            s = ((row[:, :, bit >> 3] | row[:, :, (bit >> 3) + 1] << 8) >> (bit & 7)) & ((1 << self.depth) - 1)
        elif self.depth == 10:
            s = row[:, :, 5 * (p >> 2) + (p & 3)] << 2 | (row[:, :, 5 * (p >> 2) + 4] >> (2 * (p & 3))) & 3
        else:
            s = row[:, :, 3 * (p >> 1) + (p & 1)] << 4 | (row[:, :, 3 * (p >> 1) + 2] >> (4 * (p & 1))) & 15
        return RawFrames(s.to(torch.uint16), depth=self.depth, _format=self._format)        # (one format: the unpacked frames share tone and table)

    @classmethod
    def pack(cls, frames: RawFrames, packing: str = "mipi") -> "PackedRawFrames":
        """The inverse of ``unpack`` for simulators: 10- or 12-bit ``RawFrames`` -> dense packed rows (the bits of a last group behind the last
        pixel are 0)."""
        if not isinstance(frames, RawFrames) or frames.depth not in (10, 12) or packing not in _RAW_PACKINGS:
            raise ValueError("PackedRawFrames.pack: RawFrames of depth 10 or 12 and packing 'mipi' or 'pfnc' expected")
        depth, (pixels, elements) = frames.depth, ((4, 5) if frames.depth == 10 else (2, 3))
        s = (frames.data.to(torch.int64) >> frames.lsb) & ((1 << depth) - 1)
        s = torch.nn.functional.pad(s, (0, -frames.width % pixels)).unflatten(2, (-1, pixels))                  # whole groups
        if packing == "pfnc":                                              # a group is one little-endian number of pixels * depth bits
            number = sum(s[..., k] << (depth * k) for k in range(pixels))
            data = torch.stack([(number >> (8 * i)) & 255 for i in range(elements)], dim=-1).flatten(2)[:, :, :-(-frames.width * depth // 8)]
        else:
            low = sum((s[..., k] & ((1 << (depth - 8)) - 1)) << ((depth - 8) * k) for k in range(pixels))
            data = torch.cat([s >> (depth - 8), low[..., None]], dim=-1).flatten(2)
        return cls(data.to(torch.uint8), frames.width, frames.pattern, depth, packing, frames.black, frames.gains, frames.tone)


class PackedRawStereoVideo(_StereoVideo):
    """Both views of a packed raw sensor video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor: two
    ``PackedRawFrames`` of one size, frame count, device, packing, depth, pattern, black level, white balance and tone curve.  ``len()``, slicing
    by frame range, ``to(device)`` (the packed bytes: 1.25 per pixel and view at depth 10, 1.5 at depth 12)."""
    _views = PackedRawFrames


# layout: (container, step, where R, G, B lie) of ppms_rgb_packed_format -- component indices of the pixel; for container 2 fields of its 32-bit word
_PACKED_RGB = {"rgb24": (0, 3, (0, 1, 2)), "bgr24": (0, 3, (2, 1, 0)),
               "rgba": (0, 4, (0, 1, 2)), "bgra": (0, 4, (2, 1, 0)), "argb": (0, 4, (1, 2, 3)), "abgr": (0, 4, (3, 2, 1)),
               "rgb48": (1, 3, (0, 1, 2)), "bgr48": (1, 3, (2, 1, 0)), "rgba64": (1, 4, (0, 1, 2)), "bgra64": (1, 4, (2, 1, 0)),
               "x2rgb10": (2, 1, (2, 1, 0)), "x2bgr10": (2, 1, (0, 1, 2))}
_PACKED_RGB.update({name.replace("a", "x"): _PACKED_RGB[name] for name in ("rgba", "bgra", "argb", "abgr")})      # a fourth byte that is padding: the same reads
_HWC_ORDERS = {(1, "rgb"): "rgb24", (1, "bgr"): "bgr24", (2, "rgb"): "rgb48", (2, "bgr"): "bgr48", (2, "rgba"): "rgba64", (2, "bgra"): "bgra64"}
_HWC_ORDERS.update({(1, name): name for name, (container, step, _) in _PACKED_RGB.items() if (container, step) == (0, 4)})


class PackedRGBFrames(_PackedFrames):
    """One view's N frames of interleaved RGB, (H, W, C) with the channels adjacent, as ``cv2.VideoCapture`` / ``imread``, PIL and numpy, GStreamer
    ``video/x-raw,format=BGR``, ROS ``bgr8`` / ``rgba8``, DXGI / DRM capture and ffmpeg ``rgb24`` / ``bgr0`` / ``rgb48le`` / ``x2rgb10le`` leave them:
    ``data`` (N, H0, row elements) over the caller's own buffer, ``width`` pixels wide from surface column ``x0`` (any column).  ``layout``
      "rgb24" / "bgr24": uint8, 3 bytes per pixel in that order; "rgba" = "rgbx", "bgra" = "bgrx", "argb" = "xrgb", "abgr" = "xbgr": uint8, 4 bytes
      per pixel -- the fourth is never read, whatever it holds;
      "rgb48" / "bgr48" / "rgba64" / "bgra64": ``torch.uint16`` words holding ``depth`` = 10 or 12 bits at the top (``align="msb"``, the default: the
      low bits are dropped whatever they hold) or at the bottom (``align="lsb"``: the high bits are masked);
      "x2rgb10": one little-endian 32-bit word per pixel, R in bits 29..20, G in 19..10, B in 9..0 (ffmpeg's x2rgb10le, DRM's XRGB2101010);
      "x2bgr10": R in bits 9..0, G in 19..10, B in 29..20 (DXGI's R10G10B10A2); bits 30 and 31 are ignored; ``data`` uint8 (4 bytes per pixel) or int32
      rows, its address, pitch and frame stride multiples of 4.
    (The layouts restate those projects' documentation; include/ppms.h is the definition here, and nothing has been compared with ffmpeg.)  ``data``
    may be a strided view; the class reads ``data_ptr()`` and ``stride()`` and never copies -- ``from_hwc`` takes the (N, H, W, C) tensor as it is.
    ``unpack`` is the definition of the levels: planar (N, 3, H0, W0), which ``to_rgb`` returns and ``to_float`` turns into the float video.  Not
    covered: 16-bit depth, planar high-depth RGB (gbrp10le), big-endian words, RGB565, premultiplied or meaningful alpha, float / half surfaces,
    layouts that differ between the two views, b > 1."""
    _name, _entry = "PackedRGBFrames", "ppms_video_ingest_rgb_packed"

    def __init__(self, data: torch.Tensor, width: int, layout: str = "bgr24", depth: Optional[int] = None, align: str = "msb", x0: int = 0):
        if layout not in _PACKED_RGB:
            raise ValueError(f"PackedRGBFrames: layout {layout!r}; one of {sorted(_PACKED_RGB)}")
        self.container, self.step, self.offset = _PACKED_RGB[layout]
        depths = ((8,), (10, 12), (10,))[self.container]
        if depth is None and len(depths) == 1:
            depth = depths[0]
        if depth not in depths:
            raise ValueError(f"PackedRGBFrames: depth = {depth!r} does not go with layout {layout!r}; {' or '.join(map(str, depths))}")
        self.depth = int(depth)
        self.lsb = _sample_lsb("PackedRGBFrames", align, self.depth, self.container == 1)
        self._align = (1, 2, 4)[self.container]
        dtype = (torch.uint8, torch.uint16, torch.int32 if torch.is_tensor(data) and data.dtype == torch.int32 else torch.uint8)[self.container]
        self._group = (1, 4 if (self.container, dtype) == (2, torch.uint8) else self.step)      # the elements of one pixel
        self._surface(data, width, x0, dtype, False)
        self.layout, self.align = layout, align

    @classmethod
    def from_hwc(cls, frames: torch.Tensor, order: str = "bgr", depth: Optional[int] = None, align: str = "msb") -> "PackedRGBFrames":
        """``frames`` (N, H, W, 3 | 4), uint8 or ``torch.uint16``, the channels in ``order`` ("bgr" / "rgb"; "bgra", "rgba", "argb", "abgr" and their
        x forms; 16-bit words: "rgb", "bgr", "rgba", "bgra" with ``depth`` 10 or 12) -- an OpenCV, PIL or numpy image stack as it is.  The innermost
        stride must be 1 and the pixel stride C; rows and frames may have any strides that do not overlap: a crop ``t[:, 3:40, 5:55]`` of a larger
        tensor is read where it lies.  Nothing is copied."""
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("PackedRGBFrames.from_hwc: frames must be a uint8 or uint16 tensor (N, H, W, C)")
        layout = _HWC_ORDERS.get((frames.element_size(), order))
        n, h, w, c = frames.shape
        if layout is None or _PACKED_RGB[layout][1] != c:
            raise ValueError(f"PackedRGBFrames.from_hwc: order {order!r} does not name the {c} channels of {frames.dtype} pixels; one of "
                             f"{sorted(o for es, o in _HWC_ORDERS if es == frames.element_size())}")
        if frames.stride(3) != 1 or (w > 1 and frames.stride(2) != c):
            raise ValueError(f"PackedRGBFrames.from_hwc: strides {frames.stride()}; a pixel's channels must be adjacent and the pixels of a row {c} elements apart")
        rows = torch.as_strided(frames, (n, h, w * c), (frames.stride(0), frames.stride(1), 1), frames.storage_offset())
        return cls(rows, w, layout, depth, align)

    def _row_elements(self, p: int) -> int:
        return self._group[1] * p

    def _with(self, data, x0, width) -> "PackedRGBFrames":
        return PackedRGBFrames(data, width, self.layout, self.depth, self.align, x0)

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side -- the same surface with two ``x0``.  The packed width must
        be even; a half may be odd (no pixel shares anything with its neighbour)."""
        h = self._half("split_side_by_side", self.width, False, "views")
        return self._with(self.data, self.x0, h), self._with(self.data, self.x0 + h, h)

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy."""
        h = self._half("split_top_bottom", self.height, False, "views")
        return self._like(self.data[:, :h]), self._like(self.data[:, h:])

    def format_fault(self, other: "PackedRGBFrames") -> Optional[str]:
        if (self.container, self.step, self.offset, self.depth, self.lsb) == (other.container, other.step, other.offset, other.depth, other.lsb):
            return None
        return f"the views differ in layout, depth or alignment: {(self.layout, self.depth, self.align)} and {(other.layout, other.depth, other.align)}"

    def format_struct(self) -> L.RGBPackedFormat:
        """The ``ppms_rgb_packed_format`` of these frames."""
        return L.RGBPackedFormat(self.container, self.depth, self.lsb, self.step, self.offset, 0)

    def _structs(self):
        return (self.format_struct(),)

    def table(self, device) -> torch.Tensor:
        return level_lut(device, self.depth)

    def colour_table(self, device) -> torch.Tensor:
        return colour_lut(device, self.depth)

    def levels_to_float(self, levels: torch.Tensor) -> torch.Tensor:
        return _levels_to_float(levels, self.depth)

    def unpack(self) -> torch.Tensor:
        """Planar (N, 3, H0, W0) R, G, B levels on the same device, uint8 at depth 8 and int16 in [0, 2^depth - 1] otherwise, in torch integer ops:
        the definition of the layouts on this side -- what the feature means by the levels of these frames (the kernels' operands are
        ppms_video_ingest_u8's on them, with the table of their depth) -- and the path of encoder callables of the caller."""
        p = torch.arange(self.x0, self.x0 + self.width, device=self.device)
        if self.container == 2:
            if self.data.dtype == torch.uint8:
                words = sum(self.data[:, :, 4 * p + k].to(torch.int64) << (8 * k) for k in range(4))
            else:
                words = self.data[:, :, p].to(torch.int64)
            channels = [(words >> (10 * f)) & 1023 for f in self.offset]
        else:
            # (16-bit words are gathered as the int16 with the same bits and widened to their unsigned value: uint16 tensors cannot be indexed on a GPU)
            row = self.data.view(torch.int16) if self.container == 1 else self.data
            channels = [((row[:, :, self.step * p + o].to(torch.int32) & 0xFFFF) >> self.lsb) & ((1 << self.depth) - 1) for o in self.offset]
        return torch.stack(channels, dim=1).to(torch.uint8 if self.depth == 8 else torch.int16)

    def to_rgb(self) -> torch.Tensor:
        """``unpack()``: the frames' RGB levels."""
        return self.unpack()

    def to_float(self) -> torch.Tensor:
        """float32 (N, 3, H0, W0) in [0, 255]: ``levels.float() * (255.0 / (2^depth - 1))`` (depth 8: the bytes' values) -- the video the reference
        would be given."""
        return self.levels_to_float(self.unpack())

    @classmethod
    def pack(cls, levels: torch.Tensor, layout: str = "bgr24", depth: Optional[int] = None, align: str = "msb") -> "PackedRGBFrames":
        """The inverse of ``unpack`` for simulators: planar levels (N, 3, H0, W0) as ``unpack`` gives them (uint8 for the byte layouts, int16 in
        [0, 2^depth - 1] otherwise) -> dense interleaved rows; the fourth component, spare bits of words and bits 30, 31 are 0 (the 10-bit words
        come as int32 rows)."""
        if layout not in _PACKED_RGB or not torch.is_tensor(levels) or levels.dim() != 4 or levels.shape[1] != 3:
            raise ValueError(f"PackedRGBFrames.pack: planar levels (N, 3, H0, W0) and a layout of {sorted(_PACKED_RGB)} expected")
        container, step, offset = _PACKED_RGB[layout]
        probe = cls(torch.zeros((1, 1, 4), dtype=(torch.uint8, torch.uint16, torch.int32)[container]), 1, layout, depth, align)      # (checks depth and align)
        if levels.dtype != (torch.uint8 if probe.depth == 8 else torch.int16) or bool(((levels < 0) | (levels.to(torch.int32) >> probe.depth != 0)).any()):
            raise ValueError(f"PackedRGBFrames.pack: {'uint8' if probe.depth == 8 else 'int16'} levels of {probe.depth} bits expected for layout {layout!r}")
        n, _, h, w = levels.shape
        v = levels.to(torch.int64)
        if container == 2:
            words = sum(v[:, c] << (10 * f) for c, f in enumerate(offset))
            data = words.to(torch.int32)
        else:
            pixels = torch.zeros((n, h, w, step), dtype=torch.int64, device=levels.device)
            for c, o in enumerate(offset):
                pixels[..., o] = v[:, c] << probe.lsb
            data = pixels.flatten(2).to(torch.uint8) if container == 0 else pixels.flatten(2).to(torch.int32).to(torch.uint16)
        return cls(data, w, layout, probe.depth, align)


class PackedRGBStereoVideo(_StereoVideo):
    """Both views of an interleaved RGB video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor: two
    ``PackedRGBFrames`` of one size, frame count, device, layout, depth and alignment.  ``len()``, slicing by frame range, ``to(device)`` (the
    pixels' own bytes: bgr24 3 per pixel and view, bgra and x2rgb10 4, rgb48 6); ``from_hwc`` takes a (N, 2, H, W, C) tensor as it is."""
    _views = PackedRGBFrames

    @classmethod
    def from_hwc(cls, video: torch.Tensor, order: str = "bgr", depth: Optional[int] = None, align: str = "msb") -> "PackedRGBStereoVideo":
        """``video`` (N, 2, H, W, 3 | 4): both views' ``PackedRGBFrames.from_hwc``, over the one tensor; nothing is copied."""
        if not torch.is_tensor(video) or video.dim() != 5 or video.shape[1] != 2:
            raise ValueError("PackedRGBStereoVideo.from_hwc: video must be a tensor (N, 2, H, W, C)")
        return cls(*(PackedRGBFrames.from_hwc(video[:, i], order, depth, align) for i in (0, 1)))


_BORDERS ={"replicate": L.BORDER_REPLICATE, "constant": L.BORDER_CONSTANT}


class RectifyMap:
    """One view's undistort + rectify (+ resize) map in fixed point, as ppms_video_ingest_u8_remap / _yuv420_remap / _yuv_remap read it (the arithmetic:
    include/ppms.h): for every pixel of the RECTIFIED frame H0 x W0, ``xy`` int16 (H0, W0, 2) holds the integer source coordinate (x0, y0), x
    first, and ``frac`` int16 or uint16 (H0, W0) its fraction in 1/32 pixel, fx | fy << 5 -- the layout OpenCV documents for
    ``convertMaps(..., CV_16SC2)`` (not compared with OpenCV).  ``source_size`` = (Hs, Ws) of the raw frames; ``border`` "replicate" or
    "constant" (a tap outside the frame is ``fill``, one byte for R, G and B; for sources of depth d its level ``level_fill(d)``).  Both tensors may be row-pitched views with ONE pitch
    (``xy.stride(0) == 2 * frac.stride(0)``): the class reads ``data_ptr()`` and ``stride()`` and never copies.  ``apply_levels`` is the definition
    of the remap (``apply_u8``: its depth-8 case).  Not covered: computing maps from calibration data, interpolation other than bilinear."""

    def __init__(self, xy: torch.Tensor, frac: torch.Tensor, source_size, border: str = "replicate", fill: int = 0, _checked: bool = False):
        if not torch.is_tensor(xy) or xy.dtype != torch.int16 or xy.dim() != 3 or xy.shape[2] != 2:
            raise ValueError("RectifyMap: xy must be an int16 tensor (H0, W0, 2)")
        if not torch.is_tensor(frac) or frac.dtype not in (torch.int16, torch.uint16) or frac.dim() != 2:
            raise ValueError("RectifyMap: frac must be an int16 or uint16 tensor (H0, W0)")
        h0, w0 = frac.shape
        if h0 < 1 or w0 < 1 or tuple(xy.shape[:2]) != (h0, w0):
            raise ValueError(f"RectifyMap: xy {tuple(xy.shape)} and frac {tuple(frac.shape)} must cover one non-empty frame")
        if xy.device != frac.device:
            raise ValueError("RectifyMap: xy and frac must be on one device")
        frac = frac.view(torch.int16)                               # the same 16 bits
        if xy.stride(2) != 1 or (w0 > 1 and (xy.stride(1) != 2 or frac.stride(1) != 1)):
            raise ValueError(f"RectifyMap: the last dimensions must be contiguous (xy strides {xy.stride()}, frac strides {frac.stride()})")
        # a size-1 dimension's stride is arbitrary: the smallest the kernel accepts stands in for it
        pitch = frac.stride(0) if h0 > 1 else w0
        if pitch < w0 or (h0 > 1 and xy.stride(0) != 2 * pitch):
            raise ValueError(f"RectifyMap: xy and frac need one row pitch >= W0 (xy strides {xy.stride()}, frac strides {frac.stride()})")
        if xy.data_ptr() % 4 or frac.data_ptr() % 2:
            raise ValueError("RectifyMap: xy must start at a multiple of 4 bytes, frac of 2")
        try:
            hs, ws = (int(v) for v in source_size)
        except (TypeError, ValueError):
            raise ValueError(f"RectifyMap: source_size = {source_size!r} must be (Hs, Ws)") from None
        if not (1 <= hs <= 32768 and 1 <= ws <= 32768):
            raise ValueError(f"RectifyMap: source_size = ({hs}, {ws}) must lie in 1..32768")
        if border not in _BORDERS:
            raise ValueError(f"RectifyMap: border {border!r}; one of {sorted(_BORDERS)}")
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"RectifyMap: fill = {fill} must be a byte")
        if not _checked and bool(((frac < 0) | (frac > 1023)).any()):      # once: copies made by ``to`` hold the same values
            raise ValueError("RectifyMap: frac holds values above 1023 (fx | fy << 5 with fx, fy in 0..31)")
        self.xy, self.frac, self.pitch = xy, frac, int(pitch)
        self.height, self.width, self.source_height, self.source_width = int(h0), int(w0), hs, ws
        self.border, self.fill = border, int(fill)
        self._on: Dict[torch.device, "RectifyMap"] = {xy.device: self}

    @classmethod
    def from_float(cls, map_x: torch.Tensor, map_y: torch.Tensor, source_size, border: str = "replicate", fill: int = 0) -> "RectifyMap":
        """From float source coordinates (H0, W0) per rectified pixel (what ``initUndistortRectifyMap`` gives as CV_32FC1): per coordinate
        q = round_half_even(v * 32), saturated so that q >> 5 stays an int16; then x0 = q >> 5, fx = q & 31 (floor and remainder)."""
        if not (torch.is_tensor(map_x) and torch.is_tensor(map_y) and map_x.is_floating_point() and map_y.is_floating_point()
                and map_x.dim() == 2 and map_x.shape == map_y.shape):
            raise ValueError("RectifyMap.from_float: map_x and map_y must be floating-point tensors of one shape (H0, W0)")
        if bool(torch.isnan(map_x).any()) or bool(torch.isnan(map_y).any()):
            raise ValueError("RectifyMap.from_float: a coordinate is NaN")
        qx, qy = (torch.round(m.double() * 32.0).clamp(-32768 * 32, 32767 * 32 + 31).to(torch.int64) for m in (map_x, map_y))
        xy = torch.stack([qx >> 5, qy >> 5], dim=-1).to(torch.int16)
        frac = ((qx & 31) | ((qy & 31) << 5)).to(torch.int16)
        return cls(xy, frac, source_size, border, fill, _checked=True)

    @classmethod
    def identity(cls, h: int, w: int, device=None) -> "RectifyMap":
        """The map that copies an h x w frame."""
        ys, xs = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
        return cls(torch.stack([xs, ys], dim=-1).to(torch.int16), torch.zeros((h, w), dtype=torch.int16, device=device), (h, w), _checked=True)

    @property
    def device(self) -> torch.device:
        return self.xy.device

    def to(self, device) -> "RectifyMap":
        """This map on ``device`` (6 bytes per rectified pixel, dense); made once per device and kept."""
        device = _moved_to(device)
        if device not in self._on:
            there = RectifyMap(self.xy.to(device).contiguous(), self.frac.to(device).contiguous(), (self.source_height, self.source_width), self.border,
                               self.fill, _checked=True)
            there._on = self._on
            self._on[device] = there
        return self._on[device]

    def level_fill(self, depth: int = 8) -> int:
        """``fill`` as a level of ``depth`` bits: the byte's bits repeated below it, (fill << (d - 8)) | (fill >> (16 - d)) -- 0 stays 0, 255
        becomes the top level."""
        depth = _check_depth("RectifyMap.level_fill", depth)
        return (self.fill << (depth - 8)) | (self.fill >> (16 - depth))

    def view_struct(self, depth: int = 8) -> L.RemapView:
        """The ``ppms_remap_view`` of this map for a source of ``depth`` bits."""
        return L.RemapView(self.xy.data_ptr(), self.frac.data_ptr(), self.pitch, self.source_height, self.source_width, _BORDERS[self.border],
                           self.level_fill(depth), 0)

    def apply_u8(self, rgb: torch.Tensor) -> torch.Tensor:
        """uint8 (N, 3, Hs, Ws) -> uint8 (N, 3, H0, W0) on ``rgb``'s device: the remap of include/ppms.h in torch integer ops -- what the feature
        means by the rectified bytes (the kernels' operands are ppms_video_ingest_u8's on them), and the path where the kernels cannot be used."""
        return self._apply("apply_u8", rgb, 8)

    def apply_levels(self, rgb: torch.Tensor, depth: int = 8) -> torch.Tensor:
        """The same remap on RGB levels of ``depth`` bits as ``YUVFrames.to_rgb`` gives them (uint8 at depth 8, int16 otherwise), same dtype out:
        a tap outside the frame is ``level_fill(depth)`` in constant mode, and the blend (sum w p + 512) >> 10 stays inside the levels."""
        return self._apply("apply_levels", rgb, _check_depth("RectifyMap.apply_levels", depth))

    def _apply(self, who: str, rgb: torch.Tensor, depth: int) -> torch.Tensor:
        hs, ws = self.source_height, self.source_width
        dtype, name = (torch.uint8, "uint8") if depth == 8 else (torch.int16, "int16")
        if not torch.is_tensor(rgb) or rgb.dtype != dtype or rgb.dim() != 4 or tuple(rgb.shape[1:]) != (3, hs, ws):
            raise ValueError(f"RectifyMap.{who}: {name} frames (N, 3, {hs}, {ws}) expected, got "
                             f"{tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__}")
        fill = self.level_fill(depth)
        m = self.to(rgb.device)
        x0, y0 = m.xy[..., 0].to(torch.int64), m.xy[..., 1].to(torch.int64)
        f = m.frac.to(torch.int32)
        fx, fy = f & 31, (f >> 5) & 31
        acc = torch.full((rgb.shape[0], 3, self.height, self.width), 512, dtype=torch.int32, device=rgb.device)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                cy, cx = yy.clamp(0, hs - 1), xx.clamp(0, ws - 1)
                p = rgb[:, :, cy, cx].to(torch.int32)             # clamped addresses in both modes
                if self.border == "constant":
                    p = torch.where((cy != yy) | (cx != xx), torch.full_like(p, fill), p)
                acc += ((fx if dx else 32 - fx) * (fy if dy else 32 - fy)) * p
        return (acc >> 10).to(dtype)


class StereoRectifier:
    """The two views' ``RectifyMap``s of one rig -- what ``rectify=`` of ``PPMStereo.forward`` / ``forward_batch_test`` takes: one rectified size
    (``height`` x ``width``), one source size (``source_height`` x ``source_width``), one device.  ``to(device)`` is kept per device."""

    def __init__(self, left: RectifyMap, right: RectifyMap):
        if not isinstance(left, RectifyMap) or not isinstance(right, RectifyMap):
            raise TypeError("StereoRectifier: two RectifyMaps expected")
        if (left.height, left.width) != (right.height, right.width):
            raise ValueError(f"StereoRectifier: the rectified sizes differ: {(left.height, left.width)} and {(right.height, right.width)}")
        if (left.source_height, left.source_width) != (right.source_height, right.source_width):
            raise ValueError(f"StereoRectifier: the source sizes differ: {(left.source_height, left.source_width)} and "
                             f"{(right.source_height, right.source_width)}")
        if left.device != right.device:
            raise ValueError("StereoRectifier: both maps must be on one device")
        self.left, self.right = left, right
        self.height, self.width = left.height, left.width
        self.source_height, self.source_width = left.source_height, left.source_width

    @property
    def device(self) -> torch.device:
        return self.left.device

    def to(self, device) -> "StereoRectifier":
        left, right = self.left.to(device), self.right.to(device)
        return self if left is self.left and right is self.right else StereoRectifier(left, right)

    def tensors(self):
        """The four map tensors (for record_stream)."""
        return self.left.xy, self.left.frac, self.right.xy, self.right.frac

    def apply_u8(self, left: torch.Tensor, right: torch.Tensor):
        return self.left.apply_u8(left), self.right.apply_u8(right)

    def apply_levels(self, left: torch.Tensor, right: torch.Tensor, depth: int = 8):
        return self.left.apply_levels(left, depth), self.right.apply_levels(right, depth)

    def check_source(self, who: str, h: int, w: int) -> None:
        if (int(h), int(w)) != (self.source_height, self.source_width):
            raise ValueError(f"{who}: the frames are {int(h)} x {int(w)}, the rectification maps were made for {self.source_height} x {self.source_width}")


class _FloatViews:
    """The source of a float video: ``left`` / ``right`` (n, 3, H0, W0) as the reference takes them; torch pads and normalises them.
    A source -- this class and the two below -- is what the model reads its n frames per view (b clips of n / b) of ``size`` = (H0, W0) from."""

    def __init__(self, left: torch.Tensor, right: torch.Tensor, b: int = 1):
        self.left, self.right, self.device = left, right, left.device
        self.n, self.b, self.size = int(left.shape[0]), int(b), (int(left.shape[-2]), int(left.shape[-1]))

    def float_views(self):
        """The two float32 (n, 3, H0, W0) videos for encoder callables of the caller."""
        return self.left, self.right

    def colour(self, plane: torch.Tensor, frame0: int, n: int, x0: int, y0: int, h0: int, w0: int, order: str) -> None:
        """``_ByteSource.colour`` in torch, no kernel: ``colour_bytes`` of the left frames at the clamped coordinates, on the current stream."""
        _check_colour_plane(plane, n, h0, w0)
        ys = (torch.arange(h0, device=self.device) + y0).clamp_(0, self.size[0] - 1)
        xs = (torch.arange(w0, device=self.device) + x0).clamp_(0, self.size[1] - 1)
        plane.copy_(colour_bytes(self.left[frame0:frame0 + n][:, :, ys][:, :, :, xs], order))


def _check_colour_plane(plane: torch.Tensor, n: int, h0: int, w0: int) -> None:
    if not torch.is_tensor(plane) or plane.dtype != torch.uint8 or tuple(plane.shape) != (n, h0, w0, 4) or plane.stride(3) != 1 or (w0 > 1 and plane.stride(2) != 4):
        raise ValueError(f"colour: the plane must be uint8 ({n}, {h0}, {w0}, 4) with dense pixels, got "
                         f"{(plane.dtype, tuple(plane.shape), plane.stride()) if torch.is_tensor(plane) else type(plane).__name__}")


class _ByteSource:
    """Decoded bytes of both views, optionally the RAW frames of a ``StereoRectifier`` (``size`` is then its rectified size): with this package's
    encoders ONE launch (``ingest``) rectifies, pads, normalises (the level table of the source's ``depth``) and lays out both encoders' first-layer
    operands; ``float_views`` is the path
    of other encoder callables.  The entry point and its ``_remap`` twin differ by the two maps in front of n: chosen here, once."""

    def __init__(self, entry: str, n: int, frame_size, device, rectify: Optional[StereoRectifier], b: int = 1, depth: int = 8):
        self.n, self.b, self.device, self.rectify, self.depth = int(n), int(b), device, rectify, int(depth)
        if rectify is None:
            self.size, self._entry, self._maps, self._map_tensors = (int(frame_size[0]), int(frame_size[1])), entry, (), ()
        else:
            self.size, self._entry = (rectify.height, rectify.width), entry + "_remap"
            self._maps, self._map_tensors = (rectify.left.view_struct(depth), rectify.right.view_struct(depth)), rectify.tensors()

    def ingest(self, dst_fnet: L.SP, dst_cnet: L.SP, pad_left: int, pad_top: int, h: int, w: int) -> None:
        """One launch on the current stream: both encoders' first-layer operands of the n frames, ``pad_left`` / ``pad_top`` in front, h x w."""
        L.check(getattr(L.load(), self._entry)(*self._frames(), *self._maps, self.n, *self.size, pad_left, pad_top, h, w,
                                               self._table().data_ptr(), dst_fnet, dst_cnet, L.stream_ptr()))

    def _table(self) -> torch.Tensor:
        """The level table of the launch: the float path's normalisation of every level of the source's depth (a source with a table of its own
        answers with that)."""
        return level_lut(self.device, self.depth)

    def colour(self, plane: torch.Tensor, frame0: int, n: int, x0: int, y0: int, h0: int, w0: int, order: str) -> None:
        """One launch on the current stream (the door's ppms_video_colour_* twin): ``plane`` uint8 (n, h0, w0, 4) on the device receives the left
        view as the network sees it -- pixel (f, y, x) is pixel (clamp(y + y0), clamp(x + x0)) of left frame frame0 + f, so a rectangle that
        reaches past the frame sees the replicate padding -- as "rgba8" or "bgra8" pixels: ``colour_bytes(float_views()[0], order)``, the same bits."""
        _check_colour_plane(plane, n, h0, w0)
        out = L.EgressPlane(plane.data_ptr(), plane.stride(0), plane.stride(1), _COLOUR_ORDERS[_check_colour_order("colour", order)][1], 0)
        entry = self._entry.replace("ppms_video_ingest_", "ppms_video_colour_")
        L.check(getattr(L.load(), entry)(*self._frames(), *self._maps, self.n, *self.size, frame0, n, x0, y0, h0, w0,
                                         self._colour_table().data_ptr(), C.byref(out), L.stream_ptr()))

    def _colour_table(self) -> torch.Tensor:
        """The byte table of the colour launch: ``colour_lut``'s of the source's depth (a source with a table of its own answers with that)."""
        return colour_lut(self.device, self.depth)

    def held(self):
        """The tensors the launch reads (for record_stream)."""
        return self._planes() + self._map_tensors


class _RGBBytes(_ByteSource):
    """Planar RGB bytes as ppms_video_ingest_u8 reads them: ``left`` / ``right`` uint8 (n, 3, Hs, Ws) with dense frames ``frame_stride`` bytes apart
    (two tensors, or the two views inside one window's block)."""

    def __init__(self, left: torch.Tensor, right: torch.Tensor, frame_stride: int, rectify: Optional[StereoRectifier] = None, b: int = 1):
        super().__init__("ppms_video_ingest_u8", left.shape[0], left.shape[-2:], left.device, rectify, b)
        self.left, self.right, self.frame_stride = left, right, int(frame_stride)

    def _frames(self):
        # (kept as it was: without a rectifier, two videos of ``forward`` are compared here only -- encoder callables of the caller get what they get)
        if self.right.shape != self.left.shape or self.left.shape[1] != 3:
            raise ValueError(f"PPMStereo.forward: two uint8 videos of one shape (b, T, 3, H, W) expected, got frames {tuple(self.left.shape)} and {tuple(self.right.shape)}")
        return self.left.data_ptr(), self.right.data_ptr(), self.frame_stride

    def _planes(self):
        return self.left, self.right

    def float_views(self):
        left, right = (self.left, self.right) if self.rectify is None else self.rectify.apply_u8(self.left, self.right)
        return left.float(), right.float()


class _FramePlanes(_ByteSource):
    """A stereo video of one of the frame classes: the launch is what the frames say about their door -- ``_entry`` converts the planes or packed
    rows as the decoder, camera or driver left them, reading the two ``view_struct()``s and the frames' ``_structs()``, with the frames' own level
    table (``level_lut``'s of their depth, or a raw format's tone curve)."""

    def __init__(self, video: _StereoVideo, rectify: Optional[StereoRectifier] = None):
        super().__init__(video.left._entry, len(video), (video.height, video.width), video.left.device, rectify, depth=video.depth)
        self.video = video

    def _frames(self):
        v = self.video
        return (v.left.view_struct(), v.right.view_struct(), *v.left._structs())      # host structs: read before the call returns

    def _planes(self):
        return self.video.left._tensors() + self.video.right._tensors()

    def _table(self) -> torch.Tensor:
        return self.video.left.table(self.device)

    def _colour_table(self) -> torch.Tensor:
        return self.video.left.colour_table(self.device)

    def float_views(self):
        v = self.video
        rgb = v.left.to_rgb(), v.right.to_rgb()
        left, right = rgb if self.rectify is None else self.rectify.apply_levels(*rgb, self.depth)
        return v.left.levels_to_float(left), v.right.levels_to_float(right)    # (a tone curve behind the blend, as in the kernel)


def _checked_rectifier(who: str, rectify, device, h: int, w: int) -> StereoRectifier:
    """``rectify`` for raw frames h x w on ``device`` (host frames are only measured: the maps stay where they are)."""
    rectify.check_source(who, h, w)
    return rectify.to(device) if device.type == "cuda" else rectify


def stereo_source(who: str, left, right=None, rectify: Optional[StereoRectifier] = None):
    """The source of two views -- float or uint8 tensors (b, T, 3, H, W), two ``YUVFrames``, ``RawFrames``, ``PackedYUVFrames``,
    ``PackedRawFrames`` or ``PackedRGBFrames`` -- or, with ``right`` None, of a window ``left`` of a video: a tensor (T, 2, 3, H, W), a
    ``YUVStereoVideo``, a ``RawStereoVideo``, a ``PackedYUVStereoVideo``, a ``PackedRawStereoVideo`` or a ``PackedRGBStereoVideo``.  Every argument check of the front doors is
    made here, under the name ``who``, and touches no device: rectify= reads decoded bytes (TypeError for float frames), of its source size
    (ValueError), b = 1; two ``YUVFrames`` that differ in depth, alignment or chroma subsampling, two ``RawFrames`` that differ in pattern,
    sample format, black level, gains or tone curve, or two packed views that differ in layout, packing, depth or any of those, are no stereo pair
    (ValueError); two views of different classes are none either (TypeError)."""
    if rectify is not None and not isinstance(rectify, StereoRectifier):
        raise TypeError(f"{who}: rectify must be a StereoRectifier, got {type(rectify).__name__}")
    for frames, video in ((YUVFrames, YUVStereoVideo), (RawFrames, RawStereoVideo), (PackedYUVFrames, PackedYUVStereoVideo),
                          (PackedRawFrames, PackedRawStereoVideo), (PackedRGBFrames, PackedRGBStereoVideo)):
        if isinstance(left, frames) or isinstance(right, frames):
            if not (isinstance(left, frames) and isinstance(right, frames)):
                raise TypeError(f"{who}: image1 is {type(left).__name__} and image2 is {type(right).__name__}; both views must be {frames.__name__} or both tensors")
            left, right = video(left, right), None
        if isinstance(left, video):
            if rectify is not None:
                rectify = _checked_rectifier(who, rectify, left.left.device, left.height, left.width)
            return _FramePlanes(left, rectify)
    views = (left,) if right is None else (left, right)
    for v in views:
        if not torch.is_tensor(v):
            raise TypeError(f"{who}: uint8 or float tensors, YUVFrames or a YUVStereoVideo expected, got {type(v).__name__}")
        if rectify is not None and v.dtype != torch.uint8:
            raise TypeError(f"{who}: rectify= reads decoded bytes (uint8 frames or YUVFrames), got {v.dtype}; rectify float images before the call")
    if len({v.dtype == torch.uint8 for v in views}) > 1:
        raise TypeError(f"{who}: image1 is {left.dtype} and image2 is {right.dtype}; both views must be uint8 or both floating point")
    if left.dim() != 5:
        raise ValueError(f"{who}: a video has 5 dimensions, got {tuple(left.shape)}")
    if left.dtype != torch.uint8:
        return _FloatViews(left[:, 0], left[:, 1]) if right is None else _FloatViews(left.flatten(0, 1), right.flatten(0, 1), left.shape[0])
    if rectify is not None:
        for v in views:
            rectify = _checked_rectifier(who, rectify, v.device, v.shape[-2], v.shape[-1])
    h, w = left.shape[-2:]
    if right is None:
        if left.shape[1] != 2 or left.shape[2] != 3:
            raise ValueError(f"{who}: a uint8 stereo_video is (N, 2, 3, H, W), got {tuple(left.shape)}")
        left = left.contiguous()                                 # one block: both views are read out of it, 6 * h * w bytes from frame to frame
        return _RGBBytes(left[:, 0], left[:, 1], 6 * h * w, rectify)
    if rectify is not None:
        if right.shape != left.shape or left.shape[2] != 3:
            raise ValueError(f"{who}: two uint8 videos of one shape (1, T, 3, Hs, Ws) expected, got {tuple(left.shape)} and {tuple(right.shape)}")
        if left.shape[0] != 1:
            raise NotImplementedError(f"{who}: rectify= serves b = 1")
    return _RGBBytes(left.contiguous().flatten(0, 1), right.contiguous().flatten(0, 1), 3 * h * w, rectify, left.shape[0])


def window_plan(num_ims: int, kernel_size: int = 20):
    """Sliding-window schedule of PPMStereo.forward_batch_test (ppmstereo.py:242-310): list of
    (start, stop, keep_from, keep_to) with keep_* window-local.  Trailing windows whose output the reference
    discards (:296) are not scheduled at all."""
    stride = kernel_size // 2
    if kernel_size > num_ims:
        return [(0, num_ims, 0, num_ims)]
    plan = []
    for i in range(0, num_ims, stride):
        n = min(i + kernel_size, num_ims) - i
        if plan and n >= stride:
            plan.append((i, i + n, stride // 2, n if n < kernel_size else n + (-stride // 2)))
        elif not plan:
            plan.append((i, i + n, 0, n + (-stride // 2)))
    return plan


def shard_windows(plan, rank: int, world: int):
    """Window-level sharding across GPUs (SURVEY.md section 8e level 1): windows are independent units; rank r takes
    windows r, r+world, ...  No data-path collective; the kept disparities are gathered once at the end."""
    return [w for i, w in enumerate(plan) if i % world == rank]
