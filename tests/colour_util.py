"""What the colour-out test files share (tests/test_colour_out.py without a device, tests/test_gpu_colour_out.py and
tests/test_gpu_colour_stream_order.py with one): the header's argument lists of the 13 entry points, calls of them on fake pointers THROUGH the
ingest doors' own call builders (a stand-in library hands a door's head, maps, N, H0, W0 and table to the door's colour twin), the coloured
cloud's call -- and on the GPU side one source per door, poisoned colour destinations and random colour planes.  Nothing here defines the colour:
``ppmstereo_amd.video.colour_bytes`` and ``OutputSpec.reference`` do, and the CPU file tests those two against literal values."""
import ctypes

import torch

from egress_util import GEOMETRY, IDENTITY, POISON
from ingest_util import DEV, HEADS, MAPS, rand_u8, rand_u16
from ppmstereo_amd import _lib as L

EINVAL = -1
COLOUR_TAIL = ["int N", "int H0", "int W0", "int frame0", "int n_frames", "int x0", "int y0", "int h0", "int w0", "const uint8_t* table",
               "const ppms_egress_plane* out", "void* stream"]
COLOUR_ARGS = {"ppms_video_colour_" + door + "_remap" * twin: head + MAPS * twin + COLOUR_TAIL for door, head in HEADS.items() for twin in (0, 1)}
CLOUD_COLOUR = "ppms_cloud_egress_colour"


# ---- calls on fake pointers.  Every call in the CPU file has one thing wrong with it: a call with nothing wrong would launch ---------------------
# the rectangle of the doors' own 2 frames of 37 x 50 padded to 64 x 64 at (13, 7): the whole padded frame, both frames, a pitch wider than the row
TAIL = dict(frame0=0, n_frames=2, x0=-7, y0=-13, h0=64, w0=64)
PLANE = dict(ptr=0x700000, frame_stride=64 * 260, pitch=260, format=L.FMT_RGBA8, reserved=0)


class ColourDoors:
    """Stands in for the library in the ingest test files' call builders (``test_ingest_u8._call(lib, ...)`` and the others): a call of
    ppms_video_ingest_<door> becomes the call of ppms_video_colour_<door> with the same head, maps, N, H0, W0, the ingest call's table pointer as
    the byte table, and this object's rectangle and plane.  null_plane: out == NULL."""

    def __init__(self, lib, null_plane=False, **changes):
        self.lib, self.null_plane = lib, null_plane
        self.tail = {k: changes.pop(k, v) for k, v in TAIL.items()}
        self.plane = {k: changes.pop(k, v) for k, v in PLANE.items()}
        assert not changes, changes

    def __getattr__(self, name):
        if not name.startswith("ppms_video_ingest_"):
            return getattr(self.lib, name)

        def entry(*args):
            head, (N, H0, W0, _, _, _, _, lut, _, _, stream) = args[:-11], args[-11:]
            plane = L.EgressPlane(**{**self.plane, "ptr": self.plane["ptr"] or None})
            t = self.tail
            return getattr(self.lib, name.replace("_ingest_", "_colour_"))(*head, N, H0, W0, t["frame0"], t["n_frames"], t["x0"], t["y0"], t["h0"], t["w0"], lut,
                                                                          None if self.null_plane else ctypes.byref(plane), stream)
        return entry


def call_cloud_colour(lib, null_out=False, null_colour=False, records=0x300000, frame_stride=16008, capacity=1000, index=0x400000, index_frame_stride=4004,
                      counts=0x500000, block_counts=0x600000, block_counts_len=4, q=IDENTITY, min_disp=0.25, max_uncertainty=0.5, max_depth=80.0, format=0,
                      components=4, reserved=0, colour=None, **geometry):
    """ppms_cloud_egress_colour over egress_util's geometry: 16-byte records with a capacity of 1000 and a gap between the frames, an index, and a
    "bgra8" colour plane of the 37 x 50 crop with a pitch of 204 bytes.  colour: changes of the plane's fields."""
    out = L.Cloud(records or None, frame_stride, capacity, index or None, index_frame_stride, counts or None, block_counts or None, block_counts_len,
                  (ctypes.c_float * 16)(*q), min_disp, max_uncertainty, max_depth, format, components, reserved)
    p = {**dict(ptr=0x700000, frame_stride=37 * 204, pitch=204, format=L.FMT_BGRA8, reserved=0), **(colour or {})}
    plane = L.EgressPlane(**{**p, "ptr": p["ptr"] or None})
    g = {**GEOMETRY, **geometry}
    return lib.ppms_cloud_egress_colour(g["flow"] or None, g["unc"] or None, g["T"], g["H"], g["W"], g["frame0"], g["n_frames"], g["pad_left"], g["pad_top"],
                                        g["H0"], g["W0"], None if null_out else ctypes.byref(out), None if null_colour else ctypes.byref(plane), None)


def said(lib, rc):
    """The call behind `rc` was refused; -> its message."""
    assert rc == EINVAL, rc
    return lib.ppms_last_error().decode()


# ---- with a device: one source per door, destinations, colour planes ------------------------------------------------------------------------------
def tone_curve(depth, seed):
    """A monotonic tone curve over the levels of `depth` bits with values in [0, 255], many of them near ties."""
    return torch.rand(1 << depth, generator=torch.Generator().manual_seed(seed)).sort().values * 255.0


def door_source(door, hw, seed, rectify=None, N=3):
    """The source ``stereo_source`` makes of N frames per view of size hw behind `door`: "u8", "nv12", "yuv422p12" (the largest table), "p010",
    "raw12" (grbg, black level, gains and a tone curve), "v210" (both views side by side in one surface: the right view starts inside a group) and
    "raw10p" (MIPI RAW10)."""
    from ppmstereo_amd.ppmstereo import PackedRawFrames, PackedYUVFrames, RawFrames, YUVFrames, stereo_source
    h, w = hw
    dev = lambda t: t.to(DEV)
    if door == "u8":
        return stereo_source("colour test", dev(rand_u8((N, 2, 3, h, w), seed)), rectify=rectify)
    if door == "nv12":
        views = [YUVFrames.nv12(dev(rand_u8((N, h, w), seed + i)), dev(rand_u8((N, (h + 1) // 2, (w + 1) // 2, 2), seed + 10 + i)), "bt601") for i in range(2)]
    elif door == "yuv422p12":
        views = [YUVFrames.planar(dev(rand_u16((N, h, w), seed + i, 4096)), dev(rand_u16((N, h, (w + 1) // 2), seed + 10 + i, 4096)),
                                  dev(rand_u16((N, h, (w + 1) // 2), seed + 20 + i, 4096)), 12, "422") for i in range(2)]
    elif door == "p010":
        views = [YUVFrames.p010(dev(rand_u16((N, h, w), seed + i)), dev(rand_u16((N, (h + 1) // 2, (w + 1) // 2, 2), seed + 10 + i)), full_range=True)
                 for i in range(2)]
    elif door == "raw12":
        tone = tone_curve(12, seed + 30)
        views = [RawFrames(dev(rand_u16((N, h, w), seed + i, 4096)), "grbg", 12, "lsb", black=70, gains=(1.93, 1.0, 1.52), tone=tone) for i in range(2)]
    elif door == "v210":
        assert w % 2 == 0 and w % 6 != 0
        views = PackedYUVFrames(dev(rand_u8((N, h, 16 * ((2 * w + 5) // 6)), seed)), 2 * w, "v210").split_side_by_side()
        assert views[1].x0 == w
    elif door == "raw10p":
        views = [PackedRawFrames(dev(rand_u8((N, h, 5 * ((w + 3) // 4)), seed + i)), w, "bggr", 10, "mipi", black=64, gains=(1.5, 1.0, 1.8)) for i in range(2)]
    else:
        raise KeyError(door)
    return stereo_source("colour test", *views, rectify=rectify)


class ColourDest:
    """A poisoned byte buffer holding a colour plane of n frames of h0 x w0 pixels, `lead` bytes into the allocation, rows `pitch_extra` bytes
    wider than their pixels, `frame_gap` bytes between the frames."""

    def __init__(self, n, h0, w0, pitch_extra=0, frame_gap=0, lead=0):
        self.n, self.h0, self.w0, self.lead = n, h0, w0, lead
        self.pitch = 4 * w0 + pitch_extra
        self.frame_stride = h0 * self.pitch + frame_gap
        self.buf = torch.full((lead + n * self.frame_stride + 64,), POISON, dtype=torch.uint8, device=DEV)
        self.plane = torch.as_strided(self.buf, (n, h0, w0, 4), (self.frame_stride, self.pitch, 4, 1), lead)

    def struct(self, order):
        return L.EgressPlane(self.buf.data_ptr() + self.lead, self.frame_stride, self.pitch, {"rgba8": L.FMT_RGBA8, "bgra8": L.FMT_BGRA8}[order], 0)

    def check(self, want):
        """The plane holds `want` (uint8 (n, h0, w0, 4)), and every byte outside its pixels the poison."""
        torch.cuda.synchronize()
        assert want.dtype == torch.uint8 and tuple(want.shape) == (self.n, self.h0, self.w0, 4)
        got = self.plane.cpu()
        assert torch.equal(got, want.cpu()), f"{int((got != want.cpu()).any(-1).sum())} of {self.n * self.h0 * self.w0} pixels differ"
        mask = torch.zeros_like(self.buf, dtype=torch.bool)
        torch.as_strided(mask, (self.n, self.h0, self.w0, 4), (self.frame_stride, self.pitch, 4, 1), self.lead).fill_(True)
        assert (self.buf[~mask] == POISON).all()


def padded_float(float_left, x0, y0, h0, w0):
    """float_left (n, 3, H, W) -> (n, 3, h0, w0): pixel (y, x) is pixel (clamp(y + y0), clamp(x + x0)), the replicate padding written as indexing."""
    H, W = float_left.shape[-2:]
    ys = [min(max(y + y0, 0), H - 1) for y in range(h0)]
    xs = [min(max(x + x0, 0), W - 1) for x in range(w0)]
    return float_left[:, :, ys][:, :, :, xs]


def random_colour_plane(n, h0, w0, seed, order="bgra8"):
    """uint8 (n, h0, w0, 4) with alpha 255 whose third bytes lie in 0x80..0xBF on a quarter of the pixels: there the pixel's 32 bits are the
    pattern of a signalling NaN (exponent all ones, bit 22 clear, a non-zero payload)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 256, (n, h0, w0, 4), dtype=torch.uint8, generator=g)
    c[..., 3] = 255
    quarter = torch.rand(n, h0, w0, generator=g) < 0.25
    c[..., 2] = torch.where(quarter, torch.randint(0x80, 0xC0, (n, h0, w0), dtype=torch.uint8, generator=g), c[..., 2])
    words = c.view(torch.int32)[..., 0][quarter]
    assert quarter.any() and bool((((words >> 23) & 0xFF) == 0xFF).all()) and bool((((words >> 22) & 1) == 0).all()) and bool(((words & 0x3FFFFF) != 0).any())
    return c
