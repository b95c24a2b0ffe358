"""Video out of the model: the output spec of ``forward`` / ``forward_batch_test``, a window's egress launch and the plan of the kept frames."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib as L

_PLANE_FORMATS = {"f32": (L.FMT_F32, torch.float32), "f16": (L.FMT_F16, torch.float16), "u16": (L.FMT_U16, torch.uint16), "u8": (L.FMT_U8, torch.uint8),
                  "i32": (None, torch.int32),      # (i32: the compact cloud's counts and pixel indices, no format of a plane)
                  "rgba8": (L.FMT_RGBA8, torch.uint8), "bgra8": (L.FMT_BGRA8, torch.uint8)}      # (the colour plane: 4 bytes per pixel)
_COMPONENTS = {"xyz": 3, "xyzw": 4, "xyzrgb": 4, "xyzn": 6, "xyzrgbn": 7}   # of a record, by layout ("xyzrgb" and the two with normals: the cloud only)
_CLOUD_LAYOUTS = ("xyz", "xyzw", "xyzrgb", "xyzn", "xyzrgbn")
_COLOURED, _ORIENTED = ("xyzrgb", "xyzrgbn"), ("xyzn", "xyzrgbn")       # cloud layouts whose records carry the colour word / the normal


class OutputSpec:
    """What ``forward(output=...)`` / ``forward_batch_test(output=...)`` hand back instead of float32 disparity: up to three planes that ONE
    kernel (ppms_disparity_egress, include/ppms.h) writes from the 1/4 scale's last iteration -- crop, kept frames, ``.abs()``, the 4x
    upsampling of the uncertainty and the conversion in one pass.
      disparity    "f32" | "f16" | "u16": d = |disparity| in pixels; "u16" = min(65535, rint(d * disp_scale)) (KITTI: disp_scale = 256), NaN -> 0
      depth        None | "f32" | "f16" | "u16": Z = fb / d with fb = focal_px * baseline (one fp32 product); "u16" = min(65535, rint(Z * depth_scale))
                   (baseline in metres and depth_scale = 1000: millimetres).  A pixel with d < min_disp or d = NaN is invalid: +inf in the float
                   formats, 0 in "u16".  (min_disp = 0 leaves only NaN invalid: d = 0 then gives +inf / 65535.)
      uncertainty  "f32" | "u8" | None: u = |uncertainty| in [0, 1]; "u8" = min(255, rint(u * 255)), NaN -> 0
    Every step is one fp32 operation rounded to nearest even; ``reference`` restates them in torch and is the definition the kernel is
    tested against, bit for bit.
    Keyword only, all off by default (a spec that uses none of them makes the launch above, the same bits):
      points           None | "f32" | "f16": an organised point cloud, one record per pixel of the cropped frame, result key "points" with the
                       shape (n, h0, w0, C) -- ``cv2.reprojectImageTo3D(d, Q)`` and the validity mask behind it, in the same launch
                       (ppms_scene_egress).  With x, y the pixel's column and row in the cropped plane (the image the caller fed in):
                       v_i = ((Q[i][0] * x + Q[i][1] * y) + Q[i][2] * d) + Q[i][3], X, Y, Z = v_0 / v_3, v_1 / v_3, v_2 / v_3.  "f16" is the
                       rounding to nearest even of the fp32 value (overflow: inf).
      points_layout    "xyz": C = 3 (12-byte records in f32).  "xyzw": C = 4, w = u, the upsampled |uncertainty| (16-byte records in f32, a float4).
      Q                the 4x4 reprojection matrix of the rig's calibration: anything ``torch.as_tensor`` takes with 16 elements, rounded once to
                       fp32, every entry finite.  Required with points.  ``q_matrix`` builds the one ``cv2.stereoRectify`` documents.
      max_uncertainty  None | float: a point / depth pixel with u > max_uncertainty (or u = NaN) is invalid.
      max_depth        None | float > 0: a point with Z <= 0 or Z > max_depth (or NaN), a depth pixel with fb / d > max_depth is invalid.
                       (For both gates +inf means None.)
    An invalid point carries NaN in X, Y and Z (a pixel with d < min_disp or d = NaN is one, as for depth); w is written for valid and invalid points
    alike; an invalid depth pixel is +inf (0 in "u16") as above.  The gates never touch the disparity and uncertainty planes.
      cloud            None | "f32" | "f16": the compact (unorganised) cloud -- per frame only the VALID points of the organised cloud that
                       ``points=cloud, points_layout=cloud_layout`` would give, the same bits, in row-major pixel order, stored densely from
                       record 0: what ``pts[~pts[..., 2].isnan()]`` makes of it.  Result keys "cloud" and "cloud_counts" (the number of valid
                       points per frame).  Two more launches behind the planes' launch (ppms_cloud_egress: count, place; no atomics, the order
                       is the same in every run); the planes' launch and its bits are what they are without ``cloud``.  Needs Q and a finite
                       min_disp, as points do; it may stand beside any plane and beside points (whose format and layout may differ).
      cloud_layout     "xyz" | "xyzw", as points_layout.
      cloud_index      True: result key "cloud_index", int32 y * w0 + x of every record, to gather colour or another per-pixel attribute with.
      cloud_capacity   None | int >= 1: records kept per frame.  None: h0 * w0, which can never truncate.  A frame with more valid points keeps
                       its first ``cloud_capacity`` (records and indices); "cloud_counts" still reports the full number, so the truncation shows.
      colour           None | "rgba8" | "bgra8": result key "colour", uint8 (n, h0, w0, 4) -- the LEFT view as the network saw it (converted, demosaiced,
                       white-balanced, tone-mapped, rectified), pixel-aligned with every plane above: ``video.colour_bytes`` of the source's left float
                       video, per pixel R, G, B, 255 or B, G, R, 255 (a little-endian uint32 0xFFRRGGBB, PCL's PointXYZRGB ``rgb``).  One more launch
                       (ppms_video_colour_*) behind the ingest launch; a float video makes it in torch.  A crop that reaches into the padding sees
                       the replicate padding.  Beside the organised ``points`` it is that cloud's colour.
      cloud_layout     also "xyzrgb": C = 4, the fourth 32-bit word of a record is the colour pixel at the record's (y, x), in ``colour``'s byte order
                       -- copied as an integer (ppms_cloud_egress_colour), never through a float operation.  Needs cloud="f32" and colour=.
                       ``points_layout="xyzrgb"`` does not exist (ValueError): the "colour" plane beside the points is their colour.
      colour_plane     True | False: False keeps the device plane as workspace of the "xyzrgb" cloud and leaves "colour" out of the result and of
                       the device -> host copies.  Only with cloud_layout="xyzrgb" (or "xyzrgbn").
      normals          None | "f32" | "f16": the surface normal per pixel -- a stereo SDK's NORMALS measure, what ``IntegralImageNormalEstimation`` or
                       ``estimate_normals`` make of "points" on the host --, result key "normals" with the shape (n, h0, w0, 3), from one more launch
                       (ppms_normals_egress) behind the planes' one.  A unit vector from the cross stencil (left, right, up, down) over the fp32
                       organised points of the cropped plane, whatever format ``points`` or ``cloud`` have: per direction the central difference
                       where both neighbours are usable, a one-sided one where one is; n = ty x tx, turned towards the camera, divided by its
                       length (include/ppms.h and ``reference``: every step, in order).  A neighbour is usable when it lies inside the crop, it and
                       the centre are valid points (min_disp and both gates) and it passes the jump gate.  A pixel without a tangent in either
                       direction, with an invalid centre or with a length that is 0 or not finite carries NaN in all three components.  Needs Q
                       and a finite min_disp, as points do.  Beside "points" it is that cloud's normals, record for record.
      normal_max_jump  float > 0 | None: the jump gate, |Z_N - Z_C| <= normal_max_jump * |Z_C| for neighbour N of centre C, keeps a tangent from
                       spanning a depth edge.  None or +inf: off.
      cloud_layout     also "xyzn": C = 6, X, Y, Z, nx, ny, nz in the cloud's format (PCL's PointNormal; 24-byte records in f32, 12 in f16), and
                       "xyzrgbn": C = 7, X, Y, Z, the colour word, nx, ny, nz (PointXYZRGBNormal; 28 bytes; needs cloud="f32" and colour=).  Both
                       need normals= in the cloud's format.  A record is kept iff its point AND its normal are valid; the cloud's launches
                       (ppms_cloud_egress_normals) read the normals plane, they do not recompute it.
      normals_plane    True | False: False keeps the device plane as workspace of those two clouds and leaves "normals" out of the result and of
                       the device -> host copies.  Only with cloud_layout="xyzn" or "xyzrgbn".
    What the two entry points hand back for a spec (n frames written, h0 x w0 the crop; keys in the order of ``formats``):
      ``forward(output=, crop=, frames=)``  device tensors with the batch axis of 1 in front: the planes (1, n, 1, h0, w0), "points" (1, n, h0, w0, C),
                       "normals" (1, n, h0, w0, 3), "colour" (1, n, h0, w0, 4), "cloud" (1, n, capacity, C), "cloud_counts" (1, n) int32 and
                       "cloud_index" (1, n, capacity) int32.  No float32 full-resolution tensor is made and the host is never synchronised.  Rows of
                       "cloud" / "cloud_index" past min(count, capacity) of a frame are unspecified (never written); a count above the
                       capacity tells of a truncated frame.
      ``forward_batch_test(output=)``  host tensors over the N frames of the video, pinned: each window's launches write its KEPT frames only, and only
                       those are copied device -> host, straight into their slice of the result -- uint16 disparity and uint8 confidence: 3 bytes
                       per pixel and kept frame, where the default path copies 8 for every frame of the window.  Planes (N, 1, H, W); "points"
                       (N, H, W, C), NaN where a gate or min_disp takes the pixel, 12 bytes per pixel in "xyz" f32 (``rectify=`` in front and points
                       behind need the one calibration's maps and Q); "normals" (N, H, W, 3), 12 bytes per pixel in f32 and 6 in f16; "colour"
                       (N, H, W, 4), 4 bytes per pixel.  "cloud" is a LIST of N views (min(count_f, capacity), C) of one (N, capacity, C) buffer,
                       "cloud_index" likewise (...,) int32, "cloud_counts" (N,) int64, the untruncated numbers: per window the counts are copied
                       to the host first and then only min(count_f, capacity) records of each kept frame, so by construction count_f * C *
                       element bytes cross the bus where the organised cloud moves H * W * C ("xyzrgb": 16 bytes per valid point, where "xyz" with
                       ``cloud_index`` moves 12 + 4 and leaves the gather to the host; "xyzn": 24 in f32, 12 in f16; "xyzrgbn": 28).
                       ``colour_plane=False`` / ``normals_plane=False`` keep their plane on the device.  None of this has been timed."""

    def __init__(self, disparity: str = "f32", depth: Optional[str] = None, uncertainty: Optional[str] = "f32", disp_scale: float = 256.0,
                 focal_px: Optional[float] = None, baseline: Optional[float] = None, depth_scale: float = 1000.0, min_disp: float = 2.0 ** -8,
                 *, points: Optional[str] = None, points_layout: str = "xyz", Q=None, max_uncertainty: Optional[float] = None,
                 max_depth: Optional[float] = None, cloud: Optional[str] = None, cloud_layout: str = "xyz", cloud_index: bool = False,
                 cloud_capacity: Optional[int] = None, colour: Optional[str] = None, colour_plane: bool = True, normals: Optional[str] = None,
                 normal_max_jump: Optional[float] = 0.05, normals_plane: bool = True):
        if disparity not in ("f32", "f16", "u16"):
            raise ValueError(f"OutputSpec: disparity = {disparity!r}; one of 'f32', 'f16', 'u16'")
        if depth not in (None, "f32", "f16", "u16"):
            raise ValueError(f"OutputSpec: depth = {depth!r}; None or one of 'f32', 'f16', 'u16'")
        if uncertainty not in (None, "f32", "u8"):
            raise ValueError(f"OutputSpec: uncertainty = {uncertainty!r}; None, 'f32' or 'u8'")
        f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
        self.disparity, self.depth, self.uncertainty = disparity, depth, uncertainty
        self.disp_scale, self.depth_scale, self.min_disp = f32(disp_scale), f32(depth_scale), f32(min_disp)
        if not (0.0 < self.disp_scale < math.inf):
            raise ValueError(f"OutputSpec: disp_scale = {disp_scale} must be positive and finite")
        self.focal_px, self.baseline, self.fb = focal_px, baseline, 0.0
        if depth is not None:
            if focal_px is None or baseline is None:
                raise ValueError("OutputSpec: a depth plane needs focal_px (focal length in pixels) and baseline")
            self.fb = float(torch.tensor(float(focal_px), dtype=torch.float32) * torch.tensor(float(baseline), dtype=torch.float32))
            if not (0.0 < self.fb < math.inf):
                raise ValueError(f"OutputSpec: focal_px * baseline = {self.fb} must be positive and finite")
            if not (0.0 < self.depth_scale < math.inf):
                raise ValueError(f"OutputSpec: depth_scale = {depth_scale} must be positive and finite")
            if not math.isfinite(self.min_disp):
                raise ValueError(f"OutputSpec: min_disp = {min_disp} must be finite")
        self.Q = None
        if Q is not None:
            q = torch.as_tensor(Q).detach().to("cpu", torch.float32)                            # rounded once to fp32
            if q.numel() != 16 or not torch.isfinite(q).all():
                raise ValueError(f"OutputSpec: Q must have 16 finite elements (a 4x4 reprojection matrix), got {tuple(q.shape)}: {q.flatten().tolist()}")
            self.Q = q.reshape(4, 4).clone()

        def records(name, needs, fmt, layout):           # what either record output, points or cloud, asks of its options and of the spec
            if fmt not in (None, "f32", "f16"):
                raise ValueError(f"OutputSpec: {name} = {fmt!r}; None, 'f32' or 'f16'")
            if layout not in (_CLOUD_LAYOUTS if name == "cloud" else ("xyz", "xyzw")):
                raise ValueError(f"OutputSpec: {name}_layout = {layout!r}; 'xyz' or 'xyzw'" + (" or 'xyzrgb', 'xyzn' or 'xyzrgbn'" if name == "cloud" else
                                 " (colour per point: the 'colour' plane beside the points, or cloud_layout='xyzrgb'; normals: the 'normals' plane)"))
            if fmt is not None and self.Q is None:
                raise ValueError(f"OutputSpec: {needs} Q, the 4x4 reprojection matrix of the rig's calibration (OutputSpec.q_matrix builds one)")
            if fmt is not None and not math.isfinite(self.min_disp):
                raise ValueError(f"OutputSpec: min_disp = {min_disp} must be finite")
        records("points", "points need", points, points_layout)
        records("cloud", "a cloud needs", cloud, cloud_layout)
        records("normals", "normals need", normals, "xyz")
        self.points, self.points_layout = points, points_layout
        if not isinstance(cloud_index, bool):
            raise ValueError(f"OutputSpec: cloud_index = {cloud_index!r}; True or False")
        if cloud_capacity is not None and (isinstance(cloud_capacity, bool) or not isinstance(cloud_capacity, int) or not 1 <= cloud_capacity < 2 ** 31):
            raise ValueError(f"OutputSpec: cloud_capacity = {cloud_capacity!r}; None or an int in 1 .. 2^31 - 1")
        if cloud is None and (cloud_layout != "xyz" or cloud_index or cloud_capacity is not None):
            raise ValueError("OutputSpec: cloud_layout, cloud_index and cloud_capacity describe the cloud; without cloud= they have no meaning")
        self.cloud, self.cloud_layout, self.cloud_index, self.cloud_capacity = cloud, cloud_layout, cloud_index, cloud_capacity
        if colour not in (None, "rgba8", "bgra8"):
            raise ValueError(f"OutputSpec: colour = {colour!r}; None, 'rgba8' or 'bgra8'")
        if not isinstance(colour_plane, bool):
            raise ValueError(f"OutputSpec: colour_plane = {colour_plane!r}; True or False")
        if cloud_layout in _COLOURED and (cloud != "f32" or colour is None):
            raise ValueError(f"OutputSpec: cloud_layout = {cloud_layout!r} needs cloud = 'f32' (the colour pixel is the record's fourth 32-bit word) and colour=")
        if not colour_plane and cloud_layout not in _COLOURED:
            raise ValueError("OutputSpec: colour_plane = False keeps the colour plane as the 'xyzrgb' cloud's workspace; without cloud_layout = 'xyzrgb' it has no meaning")
        self.colour, self.colour_plane = colour, colour_plane
        if not isinstance(normals_plane, bool):
            raise ValueError(f"OutputSpec: normals_plane = {normals_plane!r}; True or False")
        jump = None if normal_max_jump is None else f32(normal_max_jump)
        if jump is not None and not jump > 0.0:
            raise ValueError(f"OutputSpec: normal_max_jump = {normal_max_jump} must be positive (None or +inf: the jump gate is off)")
        if normals is None and (normal_max_jump is None or jump != f32(0.05)):
            raise ValueError("OutputSpec: normal_max_jump describes the normals; without normals= it has no meaning")
        if cloud_layout in _ORIENTED and normals != cloud:
            raise ValueError(f"OutputSpec: cloud_layout = {cloud_layout!r} needs normals= in the cloud's format {cloud!r} (a record's elements have one size), got {normals!r}")
        if not normals_plane and cloud_layout not in _ORIENTED:
            raise ValueError("OutputSpec: normals_plane = False keeps the normals plane as the 'xyzn' / 'xyzrgbn' cloud's workspace; without one of those layouts it has no meaning")
        self.normals, self.normals_plane, self.normal_max_jump = normals, normals_plane, (None if jump == math.inf else jump)       # +inf: the gate is off
        gate_u, gate_z = (None if g is None else f32(g) for g in (max_uncertainty, max_depth))
        if gate_u is not None and math.isnan(gate_u):
            raise ValueError("OutputSpec: max_uncertainty is NaN")
        if gate_z is not None and not gate_z > 0.0:
            raise ValueError(f"OutputSpec: max_depth = {max_depth} must be positive")
        self.max_uncertainty, self.max_depth = (None if g == math.inf else g for g in (gate_u, gate_z))          # +inf: the gate is off

    @staticmethod
    def q_matrix(focal_px: float, baseline: float, cx: float, cy: float, cx_right: Optional[float] = None) -> torch.Tensor:
        """The 4x4 float64 matrix ``cv2.stereoRectify`` documents as Q, for the left camera and a POSITIVE disparity (this package's d = |flow|):
        rows [1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, 1 / B, (cx_right - cx) / B]; cx_right = None: cx.  With it Z = f B / (d + cx_right - cx)
        in the baseline's unit.  A layout claim restated from OpenCV's documentation: nothing in this package is compared with OpenCV (OpenCV's own
        Q carries -1 / Tx with the sign of its translation; check the sign of Z on a rig before relying on it)."""
        f, b, cx, cy = (float(v) for v in (focal_px, baseline, cx, cy))
        if not (b != 0.0 and math.isfinite(b)):
            raise ValueError(f"OutputSpec.q_matrix: baseline = {baseline} must be finite and not 0")
        cxr = cx if cx_right is None else float(cx_right)
        return torch.tensor([[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, 1.0 / b, (cxr - cx) / b]], dtype=torch.float64)

    points_components = property(lambda self: _COMPONENTS[self.points_layout])
    cloud_components = property(lambda self: _COMPONENTS[self.cloud_layout])

    @property
    def scene(self) -> bool:
        """The spec asks for points or a gate: its launch is ppms_scene_egress (otherwise ppms_disparity_egress, as ever)."""
        return self.points is not None or self.max_uncertainty is not None or self.max_depth is not None

    def formats(self) -> Dict[str, str]:
        """{result key: format} of the requested planes, in the order disparity, depth, uncertainties, points, normals (unless normals_plane is
        False), colour (unless colour_plane is False), and of the compact cloud's arrays: cloud, cloud_counts, cloud_index."""
        cloud = self.cloud is not None
        named = (("disparity", self.disparity), ("depth", self.depth), ("uncertainties", self.uncertainty), ("points", self.points),
                 ("normals", self.normals if self.normals_plane else None),
                 ("colour", self.colour if self.colour_plane else None), ("cloud", self.cloud), ("cloud_counts", "i32" if cloud else None), ("cloud_index", "i32" if cloud and self.cloud_index else None))
        return {k: f for k, f in named if f is not None}

    def empty(self, n: int, h0: int, w0: int, device, pin_memory: bool = False, without=()) -> Dict[str, torch.Tensor]:
        """Dense (n, 1, h0, w0) tensors of the requested planes' dtypes; "points": (n, h0, w0, C); "cloud": (n, capacity, C), "cloud_counts": (n,)
        and "cloud_index": (n, capacity) int32, capacity = cloud_capacity or h0 * w0; "colour": uint8 (n, h0, w0, 4); "normals": (n, h0, w0, 3)."""
        cap = h0 * w0 if self.cloud_capacity is None else self.cloud_capacity
        special = {"points": (n, h0, w0, self.points_components), "normals": (n, h0, w0, 3), "colour": (n, h0, w0, 4), "cloud": (n, cap, self.cloud_components),
                   "cloud_counts": (n,), "cloud_index": (n, cap)}
        return {k: torch.empty(special.get(k, (n, 1, h0, w0)), dtype=_PLANE_FORMATS[f][1], device=device, pin_memory=pin_memory)
                for k, f in self.formats().items() if k not in without}      # (without: keys the caller holds tensors for already)

    @staticmethod
    def _plane(t: Optional[torch.Tensor], row_dim: int, fmt: Optional[str]) -> L.EgressPlane:
        """The ``ppms_egress_plane`` of tensor ``t``: frames along dimension 0, rows along ``row_dim``.  None: the null plane."""
        if t is None:
            return L.EgressPlane(None, 0, 0, 0, 0)
        es = t.element_size()
        return L.EgressPlane(t.data_ptr(), t.stride(0) * es, t.stride(row_dim) * es, _PLANE_FORMATS[fmt][0], 0)

    def _reprojection(self):
        """(q, max_uncertainty, max_depth) as the structs carry them: Q's 16 floats (zeros without one) and +inf for a gate that is off."""
        q = (L.c_float * 16)(*(self.Q.flatten().tolist() if self.Q is not None else [0.0] * 16))
        return (q, *(math.inf if g is None else g for g in (self.max_uncertainty, self.max_depth)))

    def struct(self, planes: Dict[str, torch.Tensor]) -> L.Egress:
        """The ``ppms_egress`` that writes into ``planes`` (dense (n, 1, h0, w0) device tensors from ``empty``)."""
        three = (self._plane(planes.get(k), 2, f) for k, f in (("disparity", self.disparity), ("depth", self.depth), ("uncertainties", self.uncertainty)))
        return L.Egress(*three, self.disp_scale, self.fb, self.depth_scale, self.min_disp)

    def scene_struct(self, planes: Dict[str, torch.Tensor]) -> L.Egress3D:
        """The ``ppms_egress3d`` that writes into ``planes`` (from ``empty``): ``struct``'s planes and constants, the (n, h0, w0, C) points, Q and
        the gates (None: +inf, off)."""
        return L.Egress3D(self.struct(planes), self._plane(planes.get("points"), 1, self.points), *self._reprojection(), self.points_components, 0)

    def cloud_struct(self, planes: Dict[str, torch.Tensor], workspace: Optional[torch.Tensor] = None) -> L.Cloud:
        """The ``ppms_cloud`` that writes into ``planes`` (from ``empty``): the (n, capacity, C) records "cloud", the (n,) "cloud_counts", the
        (n, capacity) "cloud_index" when there, Q, min_disp and the gates (None: +inf, off).  workspace: int32 device tensor of
        ppms_cloud_egress_workspace entries.  ``planes`` without "cloud": a struct with null destinations (Q, gates and format as the spec has them)."""
        t, cnt, idx = planes.get("cloud"), planes.get("cloud_counts"), planes.get("cloud_index")
        q, max_uncertainty, max_depth = self._reprojection()
        ptr = lambda x: None if x is None else x.data_ptr()
        return L.Cloud(ptr(t), 0 if t is None else t.stride(0) * t.element_size(), 0 if t is None else t.shape[1], ptr(idx),
                       0 if idx is None else idx.stride(0) * 4, ptr(cnt), ptr(workspace), 0 if workspace is None else workspace.numel(), q,
                       self.min_disp, max_uncertainty, max_depth, _PLANE_FORMATS[self.cloud or "f32"][0], self.cloud_components, 0)

    def normals_struct(self, planes: Dict[str, torch.Tensor]) -> L.Normals:
        """The ``ppms_normals`` that writes into ``planes["normals"]`` ((n, h0, w0, 3), from ``empty`` or the cloud's workspace): Q, min_disp, the
        gates and the jump gate (None: +inf, off).  ``planes`` without "normals": a struct with a null plane."""
        q, max_uncertainty, max_depth = self._reprojection()
        return L.Normals(self._plane(planes.get("normals"), 1, self.normals), q, self.min_disp, max_uncertainty, max_depth,
                         math.inf if self.normal_max_jump is None else self.normal_max_jump, 0)

    def reference(self, d: torch.Tensor, u: Optional[torch.Tensor] = None, colour: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The arithmetic of ppms_disparity_egress / ppms_scene_egress in plain torch, on CPU or device tensors of any shape: d = a float32 (signed)
        disparity, u = a float32 uncertainty at the same resolution -> the requested planes under forward_batch_test's keys.  With points, d has at
        least two dimensions and its last two are the pixel grid (row y, column x of the cropped plane); "points" has d's shape with the components
        appended -- and, for a d of four or more dimensions whose third last is 1 (the planes' (..., 1, h, w)), without that 1: (..., h, w, C).
        u is needed for an uncertainty plane, a max_uncertainty gate and the "xyzw" layout.
        With cloud, every dimension in front of the pixel grid counts frames, N in all, and three keys are made of the organised points P and their
        validity in the cloud's format and layout: "cloud", a list of N (count, C) tensors P[f][valid[f]]; "cloud_index", a list of N (count,) int32
        y * w0 + x, increasing; "cloud_counts", (N,) int64 -- the whole cloud, whatever cloud_capacity: the definition ppms_cloud_egress is tested
        against.
        colour: the uint8 (..., h, w, 4) colour plane of the same pixels (``video.colour_bytes`` of the source's left float video; the spec's
        ``colour`` names its byte order).  A spec with colour= returns it under "colour" (unless colour_plane is False), and the "xyzrgb" cloud's
        fourth component is that plane's 32 bits per pixel viewed as float32 -- the definition ppms_cloud_egress_colour is tested against.  A spec
        that needs it and gets none raises ValueError.
        With normals, "normals" has the shape of "points" with 3 components (unless normals_plane is False): the definition of include/ppms.h step by
        step over the fp32 points and their validity, every step one fp32 torch operation -- what ppms_normals_egress is tested against.  The pixel
        grid is the crop: a neighbour outside d's last two dimensions does not exist.  The "xyzn" / "xyzrgbn" cloud keeps the pixels whose point and
        normal are valid and appends the normal (in the cloud's format) to X, Y, Z[, the colour word]; "xyzrgbn" is joined as int32 words."""
        if self.colour is not None:
            if colour is None:
                raise ValueError("OutputSpec.reference: the spec has colour= and no colour plane was given")
            if colour.dtype != torch.uint8 or colour.dim() < 3 or tuple(colour.shape[-3:]) != (*d.shape[-2:], 4):
                raise ValueError(f"OutputSpec.reference: colour must be uint8 (..., {d.shape[-2]}, {d.shape[-1]}, 4), got {colour.dtype} {tuple(colour.shape)}")
        const = lambda x: torch.full((), x, dtype=torch.float32, device=d.device)

        def quant(v, scale, top, fmt):                       # min(top, rint(v * scale)), NaN -> 0: one fp32 product, ties to even
            r = torch.round(v * const(scale))
            r = torch.where(torch.isnan(r), torch.zeros_like(r), r).clamp(max=top)
            return r.to(torch.int32).to(_PLANE_FORMATS[fmt][1])

        gated = self.depth is not None or self.points is not None or self.cloud is not None or self.normals is not None
        if u is None and (self.uncertainty is not None or (gated and self.max_uncertainty is not None) or (self.points and self.points_layout == "xyzw")
                          or (self.cloud and self.cloud_layout == "xyzw")):
            raise ValueError("OutputSpec.reference: an uncertainty plane, a max_uncertainty gate or the 'xyzw' layout is requested and no uncertainty was given")
        d = d.float().abs()
        if u is not None:
            u = u.float().abs()
        out = {"disparity": d if self.disparity == "f32" else d.to(torch.float16) if self.disparity == "f16" else quant(d, self.disp_scale, 65535.0, "u16")}
        if gated:
            ok = d >= const(self.min_disp)                   # (false for NaN)
            if self.max_uncertainty is not None:
                ok = ok & (u <= const(self.max_uncertainty))                     # (false for NaN)
        if self.depth is not None:
            z = const(self.fb) / d                           # tensor / tensor: a correctly rounded fp32 division
            valid = ok if self.max_depth is None else ok & (z <= const(self.max_depth))
            z = torch.where(valid, z, const(math.inf))
            if self.depth == "u16":
                out["depth"] = torch.where(valid, quant(z, self.depth_scale, 65535.0, "u16").to(torch.int32), 0).to(torch.uint16)
            else:
                out["depth"] = z if self.depth == "f32" else z.to(torch.float16)
        if self.uncertainty is not None:
            out["uncertainties"] = u if self.uncertainty == "f32" else quant(u, 255.0, 255.0, "u8")
        with_colour = self.colour is not None and self.colour_plane       # ("colour" stands behind "points" and "normals", as in ``formats``)
        keep = None
        if self.points is not None or self.cloud is not None or self.normals is not None:
            if d.dim() < 2:
                raise ValueError(f"OutputSpec.reference: points take the pixel grid from d's last two dimensions, got {tuple(d.shape)}")
            x = torch.arange(d.shape[-1], dtype=torch.float32, device=d.device)
            y = torch.arange(d.shape[-2], dtype=torch.float32, device=d.device)[:, None]
            q = self.Q.to(d.device)
            v = [((q[i, 0] * x + q[i, 1] * y) + q[i, 2] * d) + q[i, 3] for i in range(4)]       # one fp32 operation each, in this order
            xyz = [v[i] / v[3] for i in range(3)]
            valid = ok if self.max_depth is None else ok & (xyz[2] > 0) & (xyz[2] <= const(self.max_depth))
            squeeze = lambda t: t.squeeze(-4) if d.dim() >= 4 and d.shape[-3] == 1 else t          # (the planes' (..., 1, h, w) -> (..., h, w, C))

            def organised(fmt, layout):                  # the organised cloud in one format and layout
                comps = [torch.where(valid, c, const(math.nan)) for c in xyz] + ([u.expand_as(d)] if layout == "xyzw" else [])
                pts = squeeze(torch.stack(comps, dim=-1))
                return pts if fmt == "f32" else pts.to(torch.float16)

            if self.points is not None:
                out["points"] = organised(self.points, self.points_layout)
            keep = valid
            if self.normals is not None:                 # include/ppms.h, steps 1 to 5: one fp32 operation each, in that order
                h, w = d.shape[-2:]

                def at(t, dy, dx):                       # t at (y + dy, x + dx); outside the crop: 0 / False (such a neighbour is never usable)
                    o = torch.zeros_like(t)
                    o[..., max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = t[..., max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)]
                    return o

                def tangent(dy, dx):                     # plus side (dy, dx), minus side (-dy, -dx): (the three differences, a tangent exists)
                    use = []
                    for sy, sx in ((dy, dx), (-dy, -dx)):
                        ok_n = at(valid, sy, sx) & valid
                        if self.normal_max_jump is not None:
                            ok_n = ok_n & ((at(xyz[2], sy, sx) - xyz[2]).abs() <= const(self.normal_max_jump) * xyz[2].abs())
                        use.append(ok_n)
                    return [torch.where(use[0], at(c, dy, dx), c) - torch.where(use[1], at(c, -dy, -dx), c) for c in xyz], use[0] | use[1]

                (tx, has_x), (ty, has_y) = tangent(0, 1), tangent(1, 0)
                n = [ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]]
                flip = ((n[0] * xyz[0] + n[1] * xyz[1]) + n[2] * xyz[2]) > 0                       # towards the origin
                n = [torch.where(flip, -c, c) for c in n]
                # the correctly rounded fp32 square root, whatever the host's vector math does: taken in float64 and rounded once (53 >= 2 * 24 + 2
                # bits: the double rounding is innocuous).  torch's own fp32 sqrt on a CPU is a vector library's, off by one ulp now and then.
                length = torch.sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).double()).float()
                keep = valid & has_x & has_y & (length > 0) & torch.isfinite(length)              # the normal is valid
                normals = squeeze(torch.stack([torch.where(keep, c / length, const(math.nan)) for c in n], dim=-1))
                if self.normals_plane:
                    out["normals"] = normals if self.normals == "f32" else normals.to(torch.float16)
        if with_colour:
            out["colour"] = colour
        if self.cloud is not None:                      # per frame (every dimension in front of the pixel grid counts frames): the valid records
            if self.cloud_layout not in _ORIENTED:
                keep = valid
            if self.cloud_layout in _COLOURED:           # X, Y, Z, the colour pixel's 32 bits [and the normal], joined and selected as int32 words:
                xyz32 = organised("f32", "xyz").contiguous().view(torch.int32)                     # no float operation ever sees the colour word
                words = colour.contiguous().view(torch.int32).reshape(*xyz32.shape[:-1], 1)
                pts = torch.cat([xyz32, words] + ([normals.contiguous().view(torch.int32)] if self.cloud_layout == "xyzrgbn" else []), dim=-1)
            elif self.cloud_layout == "xyzn":
                pts = torch.cat([organised(self.cloud, "xyz"), normals if self.cloud == "f32" else normals.to(torch.float16)], dim=-1)
            else:
                pts = organised(self.cloud, self.cloud_layout)
            pts, keep = pts.reshape(-1, pts.shape[-3] * pts.shape[-2], pts.shape[-1]), keep.reshape(-1, d.shape[-2] * d.shape[-1])
            out["cloud"] = [p[k].view(torch.float32) if p.dtype == torch.int32 else p[k] for p, k in zip(pts, keep)]
            out["cloud_index"] = [k.nonzero().flatten().to(torch.int32) for k in keep]      # y * w0 + x, increasing
            out["cloud_counts"] = keep.sum(dim=1)    # int64: the full numbers, whatever cloud_capacity
        return out


class _EgressCall:
    """One egress launch as ``cascade`` makes it: the spec, the crop (pad_left, pad_top, H0, W0) inside the padded frame (None: the whole
    frame) and the window-local frame range (None: all frames)."""

    def __init__(self, spec: OutputSpec, crop=None, frames=None):
        if not isinstance(spec, OutputSpec):
            raise TypeError(f"output must be an OutputSpec, got {type(spec).__name__}")
        self.spec, self.crop, self.frames = spec, (None if crop is None else tuple(int(x) for x in crop)), (None if frames is None else tuple(int(x) for x in frames))
        self.colour: Optional[torch.Tensor] = None               # the colour plane of this call's region, written in front of the encoders (``fill_colour``)

    def region(self, T: int, H: int, W: int):
        """(pad_left, pad_top, h0, w0, f0, f1) of this call in a window of T padded frames H x W."""
        pad_left, pad_top, h0, w0 = (0, 0, H, W) if self.crop is None else self.crop
        f0, f1 = (0, T) if self.frames is None else self.frames
        if not 0 <= f0 < f1 <= T:
            raise ValueError(f"output: frames = {(f0, f1)} is no range inside the window's {T} frames")
        return pad_left, pad_top, h0, w0, f0, f1

    def fill_colour(self, source, T: int, H: int, W: int, pad_left: int, pad_top: int) -> None:
        """A spec with colour=: allocates the (n, h0, w0, 4) colour plane of this call's region on the current stream and enqueues ``source.colour``
        there (one launch; a float video: torch ops).  ``pad_left`` / ``pad_top``: what the ingest of the T frames to H x W put in front, so the
        crop's pixel (y, x) is source pixel (y + crop_top - pad_top, x + crop_left - pad_left), clamped: the replicate padding the network saw."""
        if self.spec.colour is None:
            return
        crop_left, crop_top, h0, w0, f0, f1 = self.region(T, H, W)
        self.colour = torch.empty((f1 - f0, h0, w0, 4), dtype=torch.uint8, device=source.device)
        source.colour(self.colour, f0, f1 - f0, crop_left - pad_left, crop_top - pad_top, h0, w0, self.spec.colour)

    def launch(self, eng) -> Dict[str, torch.Tensor]:
        """Allocates the planes on the current stream and enqueues the launch there, behind the engine's last iteration.  A spec with a cloud adds
        "cloud" (n, capacity, C), "cloud_counts" (n,) and "cloud_index" (n, capacity) when asked; rows of "cloud" and "cloud_index" past
        min(count, capacity) of their frame are unspecified (never written).  A spec with colour= puts the plane ``fill_colour`` wrote into the
        result ("colour"; not with colour_plane=False) and hands it to the "xyzrgb" cloud's launches (ppms_cloud_egress_colour).  A spec with
        normals= adds ppms_normals_egress's launch between the planes' and the cloud's and "normals" (n, h0, w0, 3) (not with normals_plane=False);
        the "xyzn" / "xyzrgbn" cloud's launches (ppms_cloud_egress_normals) read that plane."""
        spec = self.spec
        pad_left, pad_top, h0, w0, f0, f1 = self.region(eng.T, 4 * eng.h, 4 * eng.w)
        planes = spec.empty(f1 - f0, h0, w0, eng.FLOW_OUT.device, without=("colour",))
        if spec.colour is not None:
            if self.colour is None or tuple(self.colour.shape) != (f1 - f0, h0, w0, 4):
                raise RuntimeError("output: the spec has colour= and no colour plane of this call's region was written (fill_colour) in front of the cascade")
            self.colour.record_stream(torch.cuda.current_stream())      # allocated on the caller's stream, read by the cloud's launch here
            if spec.colour_plane:
                planes = {k: (self.colour if k == "colour" else planes[k]) for k in spec.formats()}
        out = spec.scene_struct(planes) if spec.scene else spec.struct(planes)      # ppms_scene_egress / ppms_disparity_egress
        eng.egress(out, f0, f1 - f0, pad_left, pad_top, h0, w0)
        normals = None
        if spec.normals is not None:                             # ppms_normals_egress: one launch behind the planes' one, in front of the cloud's
            normals = planes["normals"] if spec.normals_plane else torch.empty((f1 - f0, h0, w0, 3), dtype=_PLANE_FORMATS[spec.normals][1],
                                                                                device=eng.FLOW_OUT.device)      # (the oriented cloud's workspace)
            eng.egress(spec.normals_struct({"normals": normals}), f0, f1 - f0, pad_left, pad_top, h0, w0)
        if spec.cloud is not None:                               # ppms_cloud_egress: two more launches behind the planes' one, on the same stream
            oriented = spec.cloud_layout in _ORIENTED            # (ppms_cloud_egress_normals: its workgroups and its workspace are its own)
            query = L.load().ppms_cloud_egress_normals_workspace if oriented else L.load().ppms_cloud_egress_workspace
            workspace = torch.empty(query(f1 - f0, h0, w0), dtype=torch.int32, device=eng.FLOW_OUT.device)
            colour = spec._plane(self.colour, 1, spec.colour) if spec.cloud_layout in _COLOURED else None
            eng.egress(spec.cloud_struct(planes, workspace), f0, f1 - f0, pad_left, pad_top, h0, w0, colour,
                       spec._plane(normals, 1, spec.normals) if oriented else None)
        return planes


def egress_plan(plan):
    """``window_plan`` with the destination of every window's kept frames: (start, stop, keep_from, keep_to, dst_from, dst_to) -- the egress
    launch of the window writes its frames [keep_from, keep_to), and they are frames [dst_from, dst_to) of the video."""
    return [(start, stop, keep_from, keep_to, start + keep_from, start + keep_to) for start, stop, keep_from, keep_to in plan]


# ------------------------------------------------------------------ the sinks of forward_batch_test: what becomes of a window's result
# take(result, padder, keep_from, keep_to, dst_from, dst_to) per window -- the window's ``_forward_images`` result, the InputPadder that crops it
# back and its span of ``egress_plan`` --, result() once behind the last window: the dict the call returns.

def _idle_stream(device) -> None:
    # device -> host.  The stream is synchronised FIRST (a spinning wait): a pageable copy issued while the clip's ~900 launches are
    # still queued blocks inside the runtime on an interrupt-driven wait, and on a loaded host (the GPU boxes: load average 50-60)
    # the thread was rescheduled 50-150 ms late in every other call (whole call 50 / 100 / 195 ms alternating; with the
    # synchronisation in front the copy finds an idle stream: 49-50 ms every time, tools/whole_call_probe.py)
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


class _Float32Sink:
    """The default: the window's float32 (disparity, uncertainty), each (1, T, 1, H, W), unpadded and copied to the host in one piece."""

    def __init__(self):
        self.kept = ([], [])

    def take(self, result, padder, keep_from, keep_to, dst_from, dst_to):
        du = torch.cat([padder.unpad(x[0])[:, None] for x in result])                                     # one copy for both results
        _idle_stream(du.device)
        du = du.cpu()
        for kept, x in zip(self.kept, du.chunk(2)):
            kept.append(x[keep_from:keep_to])

    def result(self) -> Dict[str, torch.Tensor]:
        return {key: torch.cat(kept).squeeze(1).abs()[:, :1] for key, kept in zip(("disparity", "uncertainties"), self.kept)}


class _PlaneSink:
    """output=: the planes a window's egress launches wrote for its kept frames, each (1, n, ...), copied straight into their slice of host
    buffers allocated once (pinned by default).  Per frame only the records of the compact cloud that exist are copied."""
    RAGGED = ("cloud", "cloud_index")

    def __init__(self, spec: OutputSpec, n: int, h0: int, w0: int, pin_memory: bool = True):
        self.host = spec.empty(n, h0, w0, "cpu", pin_memory=pin_memory)

    def take(self, planes, padder, keep_from, keep_to, dst_from, dst_to):
        host, ragged = self.host, [key for key in self.RAGGED if key in planes]
        _idle_stream(next(iter(planes.values())).device)
        for key, plane in planes.items():
            if key not in ragged:
                host[key][dst_from:dst_to].copy_(plane[0])             # kept frames only, device -> their slice of the result
        if ragged:                                                     # the counts are on the host now: min(count, capacity) records per kept frame
            for i, count in enumerate(host["cloud_counts"][dst_from:dst_to].tolist()):
                for key in ragged:
                    k = min(count, planes[key].shape[2])
                    host[key][dst_from + i, :k].copy_(planes[key][0, i, :k])

    def result(self) -> Dict:
        host = self.host
        if "cloud" in host:                                            # views of the buffers: no row past a frame's records exists
            counts = host["cloud_counts"].tolist()
            for key in self.RAGGED:
                if key in host:
                    host[key] = [host[key][f, :min(c, host[key].shape[1])] for f, c in enumerate(counts)]
            host["cloud_counts"] = host["cloud_counts"].to(torch.int64)                      # the untruncated numbers
        return host


class _KeptOnDevice:
    """shard_ranks: this rank's kept float32 frames stay on the device, each piece with its first frame in video coordinates, and every rank
    gets the video in one gather at the end (``dist.gather_kept_frames``)."""

    def __init__(self, n: int, h0: int, w0: int):
        self.kept, self.shape = ([], []), (n, h0, w0)

    def take(self, result, padder, keep_from, keep_to, dst_from, dst_to):
        for kept, x in zip(self.kept, result):
            kept.append((dst_from, padder.unpad(x[0])[keep_from:keep_to].abs()[:, :1]))      # (n, 1, H0, W0)

    def result(self) -> Dict[str, torch.Tensor]:
        from .dist import gather_kept_frames
        disp, unc = (gather_kept_frames(kept, *self.shape) for kept in self.kept)
        return {"disparity": disp.cpu(), "uncertainties": unc.cpu()}
