"""What the ingest test files share (tests/test_ingest_*.py without a device, tests/test_gpu_ingest_*.py with one): the library, the header's argument
lists, calls through the C ABI on fake pointers, random samples, the integer restatement of the remap -- and on the GPU side the float path's
operands, fresh destinations and the model.  The restatements of each format's own arithmetic (float64_rgb, restated_levels ...) stay in the file
of that format: they are the oracles, and nothing here comes from ppmstereo_amd.video."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from ppmstereo_amd import _lib as L
    return L.load()


def header_args(name):
    """The argument list of `name` as include/ppms.h declares it."""
    src = open(os.path.join(ROOT, "include", "ppms.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppms.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- the ABI of the 12 entry points and the 5 size exports, as include/ppms.h states it -----------------------------------------------------------
_VIEWS = {"yuv": "const ppms_yuv_view*", "raw": "const ppms_raw_view*", "packed": "const ppms_packed_view*"}
_head = lambda view, *rest: [f"{_VIEWS[view]} left", f"{_VIEWS[view]} right", *rest]
HEADS = {"u8": ["const uint8_t* left", "const uint8_t* right", "int64_t frame_stride"],
         "yuv420": _head("yuv", "const ppms_yuv_matrix* m"),
         "yuv": _head("yuv", "const ppms_yuv_matrix* m", "const ppms_yuv_format* fmt"),
         "raw": _head("raw", "const ppms_raw_format* fmt"),
         "yuv_packed": _head("packed", "const ppms_yuv_matrix* m", "const ppms_yuv_packed_format* fmt"),
         "raw_packed": _head("packed", "const ppms_raw_packed_format* fmt")}
MAPS = ["const ppms_remap_view* lmap", "const ppms_remap_view* rmap"]
TAIL = ["int N", "int H0", "int W0", "int pad_left", "int pad_top", "int H", "int W", "const float* lut", "ppms_sp dst_fnet", "ppms_sp dst_cnet", "void* stream"]
ENTRY_ARGS = {"ppms_video_ingest_" + door + "_remap" * twin: head + MAPS * twin + TAIL for door, head in HEADS.items() for twin in (0, 1)}
# size export: (its arguments, the ctypes structs it measures, their sizes)
SIZE_EXPORTS = {"ppms_yuv_struct_sizes": (["int* view", "int* matrix"], ("YUVView", "YUVMatrix"), (56, 32)),
                "ppms_yuv_format_struct_size": (["int* fmt"], ("YUVFormat",), (32,)),
                "ppms_remap_struct_size": (["int* view"], ("RemapView",), (40,)),
                "ppms_raw_struct_sizes": (["int* view", "int* format"], ("RawView", "RawFormat"), (24, 48)),
                "ppms_packed_struct_sizes": (["int* view", "int* yuv_format", "int* raw_format"], ("PackedView", "YUVPackedFormat", "RawPackedFormat"), (24, 32, 48))}
# struct: (its fields in the header's order, the offsets of those behind the first 64-bit member or array)
FIELDS = {"YUVView": (["y", "u", "v", "frame_stride_y", "frame_stride_c", "pitch_y", "pitch_c", "step_c", "reserved"], {}),
          "YUVMatrix": (["y_off", "cy", "crv", "cgu", "cgv", "cbu", "shift", "reserved"], {}),
          "YUVFormat": (["sample_bytes", "depth", "lsb", "sub_x", "sub_y", "reserved"], {}),
          "RemapView": (["xy", "frac", "pitch", "hs", "ws", "border", "fill", "reserved"], {}),
          "RawView": (["data", "frame_stride", "pitch", "reserved"], dict(frame_stride=8, pitch=16, reserved=20)),
          "RawFormat": (["sample_bytes", "depth", "lsb", "pattern", "black", "gain", "shift", "reserved"], dict(gain=20, shift=32, reserved=36)),
          "PackedView": (["data", "frame_stride", "pitch", "x0"], dict(frame_stride=8, pitch=16, x0=20)),
          "YUVPackedFormat": (["container", "depth", "lsb", "order", "reserved"], dict(reserved=16)),
          "RawPackedFormat": (["packing", "depth", "pattern", "black", "gain", "shift", "reserved"], dict(gain=16, shift=28, reserved=32))}


def ctype_of(arg):
    """The ctypes type that binds the header's argument `arg` ("const ppms_raw_view* left")."""
    from ppmstereo_amd import _lib as L
    struct = {"yuv_view": L.YUVView, "yuv_matrix": L.YUVMatrix, "yuv_format": L.YUVFormat, "raw_view": L.RawView, "raw_format": L.RawFormat,
              "packed_view": L.PackedView, "yuv_packed_format": L.YUVPackedFormat, "raw_packed_format": L.RawPackedFormat, "remap_view": L.RemapView}
    plain = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "ppms_sp": L.SP, "const float*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p,
             "void*": ctypes.c_void_p, "int*": ctypes.POINTER(ctypes.c_int)}
    plain.update({f"const ppms_{k}*": ctypes.POINTER(v) for k, v in struct.items()})
    return plain[arg.rsplit(" ", 1)[0]]


# ---- calls on fake pointers: pointers into device memory are never dereferenced on the host, every check comes before the launch --------------
def yuv_view(y, u, v, fsy, fsc, pitch_y, pitch_c, step_c, reserved=0):
    from ppmstereo_amd import _lib as L
    return L.YUVView(y or None, u or None, v or None, fsy, fsc, pitch_y, pitch_c, step_c, reserved)


def raw_view(data, fs, pitch, reserved=0):
    from ppmstereo_amd import _lib as L
    return L.RawView(data or None, fs, pitch, reserved)


def packed_view(data=0x100000, fs=37 * 256, pitch=256, x0=0):
    from ppmstereo_amd import _lib as L
    return L.PackedView(data or None, fs, pitch, x0)


def remap_view(xy=0x400000, frac=0x500000, pitch=50, hs=37, ws=50, border=0, fill=0, reserved=0):
    from ppmstereo_amd import _lib as L
    return L.RemapView(xy or None, frac or None, pitch, hs, ws, border, fill, reserved)


def call(lib, entry, head, maps=(), null=(), null_maps=(), N=2, H0=37, W0=50, pad_left=7, pad_top=13, H=64, W=64, lut=0x3000, fnet=True, cnet=True):
    """lib.<entry>(*head, *maps, N, ..., stream): structs of `head` and `maps` go by reference (an index in `null` / `null_maps`: NULL instead), plain
    values as they are; 0 for `lut` is NULL, and a destination that is off has hi == NULL."""
    from ppmstereo_amd import _lib as L
    ref = lambda xs, nulls: [None if i in nulls else (ctypes.byref(x) if isinstance(x, ctypes.Structure) else x) for i, x in enumerate(xs)]
    sp = lambda on, c: L.SP(0x10000 if on else None, 0x20000 if on else None, c, c)
    return getattr(lib, entry)(*ref(head, null), *ref(maps, null_maps), N, H0, W0, pad_left, pad_top, H, W, lut or None, sp(fnet, 32), sp(cnet, 64), None)


def call_twin(lib, entry, head, null=(), lmap=None, rmap=None, null_rmap=False, **geometry):
    """`call` of `entry` -- or, with lmap / rmap (dicts: fields of remap_view over border = 1) or null_rmap, of its _remap twin."""
    if lmap is None and rmap is None and not null_rmap:
        return call(lib, entry, head, null=null, **geometry)
    maps = [remap_view(**{"border": 1, **(m or {})}) for m in (lmap, rmap)]
    return call(lib, entry + "_remap", head, maps, null=null, null_maps=(1,) if null_rmap else (), **geometry)


def sized_maps(bad):
    """lmap / rmap of the _remap twin whose source frame is the case's own H0 x W0."""
    m = dict(hs=bad.get("H0", 37), ws=bad.get("W0", 50))
    return dict(lmap=m, rmap=m)


def not_about_the_maps(bad):
    """The case names no map, and its frame is one a map can name as its source frame (hs, ws >= 1)."""
    return not {"lmap", "rmap", "null_rmap"} & set(bad) and bad.get("H0", 1) >= 1 and bad.get("W0", 1) >= 1


def one_message(lib, door, plain, twin, bad):
    """The rule of the doors: whatever is wrong with a call that is not about the maps, the plain entry and its _remap twin refuse it with one code
    and one message.  The twin reads its frames' size from the maps and calls it hs x ws, the frames "source" frames: the only words that may differ."""
    said = []
    for entry in (plain, twin):
        lib.ppms_mem_attn_splits(3, 3, 256, 1)                  # (a successful call in between: the message below is this call's)
        assert entry(lib, **bad) == EINVAL, bad
        said.append(lib.ppms_last_error().decode())
    (name, text), (twin_name, twin_text) = (m.split(": ", 1) for m in said)
    assert twin_name == name + "_remap" and name == "video_ingest_" + door
    assert re.sub(r"\bws\b", "W0", re.sub(r"\bhs\b", "H0", twin_text)).replace("a source frame's", "a frame's") == text, said


def refused(lib, rc, *about):
    """The call behind `rc` was refused, and its message speaks of every one of `about`; -> the message."""
    msg = lib.ppms_last_error()
    assert rc == EINVAL and msg and all(a.encode() in msg for a in about), (rc, about, msg)
    return msg


def rand_u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def rand_u16(shape, seed, top=1 << 16):
    return torch.randint(0, top, shape, dtype=torch.int32, generator=torch.Generator().manual_seed(seed)).to(torch.uint16)


# ---- the remap's arithmetic, restated ----------------------------------------------------------------------------------------------------------
def restated_remap(rgb, xy, frac, border="replicate", fill=0, top=255):
    """rgb (N, 3, Hs, Ws) levels in [0, top] (uint8, or int16 for deeper levels), xy (H0, W0, 2) int16, frac (H0, W0) 16-bit -> (N, 3, H0, W0) of
    rgb's dtype by the header's formula, written on flat pixel indices with torch.gather and a floor division (not RectifyMap.apply_levels'
    indexing and shift)."""
    N, _, hs, ws = rgb.shape
    H0, W0 = frac.shape
    flat = rgb.reshape(N, 3, hs * ws).to(torch.int64)
    x0, y0 = xy[..., 0].reshape(-1).to(torch.int64), xy[..., 1].reshape(-1).to(torch.int64)
    f = frac.reshape(-1).to(torch.int64) & 0xFFFF
    fx, fy = f % 32, (f // 32) % 32
    weights = [(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy]
    assert bool((sum(weights) == 1024).all())
    total = torch.zeros((N, 3, H0 * W0), dtype=torch.int64, device=rgb.device)
    for (dy, dx), w in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < hs) & (xx >= 0) & (xx < ws)
        index = torch.minimum(torch.maximum(yy, torch.zeros_like(yy)), torch.full_like(yy, hs - 1)) * ws + \
            torch.minimum(torch.maximum(xx, torch.zeros_like(xx)), torch.full_like(xx, ws - 1))
        tap = torch.gather(flat, 2, index.expand(N, 3, -1))
        if border == "constant":
            tap = tap * inside + fill * (~inside)
        total += w * tap
    out = torch.div(total + 512, 1024, rounding_mode="floor")
    assert int(out.min()) >= 0 and int(out.max()) <= top          # no clamp is needed
    return out.to(rgb.dtype).reshape(N, 3, H0, W0)


# ---- with a device: the float path's operands, destinations, the doors through ctypes, the model ------------------------------------------------
DEV = "cuda:0"


def patterned(pixels, channels):
    """A destination whose every 16-bit word is non-zero before the launch (so the zeroed tail channels are seen to be written)."""
    from ppmstereo_amd import _lib as L
    t = L.SPTensor(pixels, channels, DEV, zero=False)
    t.data.view(torch.int16).copy_((torch.arange(t.data.numel(), device=DEV) % 251 + 1).to(torch.int16).view(t.data.shape))
    return t


def fresh(N, H, Wd):
    """Both destinations of N frames per view padded to H x Wd."""
    return patterned(2 * N * (H // 2) * (Wd // 2), 32), patterned(N * (H // 4) * (Wd // 4), 64)


def bits(t):
    return t.data.view(torch.int16)


def float_path_operands(left_u8, right_u8, pad):
    """left / right (N, 3, H0, W0) uint8 on the device, pad = F.pad's [left, right, top, bottom] -> the k = 2 operand of cat([left, right])
    and the k = 4 operand of left, as the float path produces them."""
    from ppmstereo_amd import _lib as L
    lib = L.load()
    l, r = left_u8.float(), right_u8.float()
    if any(pad):
        l, r = (torch.nn.functional.pad(x, pad, mode="replicate") for x in (l, r))
    im1, im2 = (2 * (l / 255.0) - 1.0).contiguous(), (2 * (r / 255.0) - 1.0).contiguous()
    N, _, H, Wd = im1.shape
    both = torch.cat([im1, im2], dim=0).contiguous()
    f, c = fresh(N, H, Wd)
    L.check(lib.ppms_img_s2d(both.data_ptr(), f.view(), 2 * N, 3, H, Wd, 2, L.stream_ptr()))
    L.check(lib.ppms_img_s2d(im1.data_ptr(), c.view(), N, 3, H, Wd, 4, L.stream_ptr()))
    return f, c, H, Wd


def ingest_door(entry, head, maps, n, size, pad_left, pad_top, H, Wd, lut, fview, cview):
    """ppms_video_ingest_<entry>(*head, n, *size, ...) on the device, or with `maps` (the two views' RectifyMaps, whose rectified size replaces
    `size`) its _remap twin; the table `lut` says the depth of the levels."""
    from ppmstereo_amd import _lib as L
    if maps is None:
        name, frames = entry, (n, *size)
    else:
        depth = {256: 8, 1024: 10, 4096: 12}[lut.numel()]
        name, frames = entry + "_remap", (maps[0].view_struct(depth), maps[1].view_struct(depth), n, maps[0].height, maps[0].width)
    with torch.cuda.device(DEV):
        rc = getattr(L.load(), "ppms_video_ingest_" + name)(*head, *frames, pad_left, pad_top, H, Wd, lut.data_ptr(), fview, cview, L.stream_ptr())
    L.check(rc)
    return rc


def ingest(left, right, stride, N, H0, W0, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The uint8 door on two device pointers to planar RGB frames `stride` bytes apart."""
    from ppmstereo_amd.ppmstereo import byte_lut
    return ingest_door("u8", (left, right, stride), maps, N, (H0, W0), pad_left, pad_top, H, Wd, byte_lut(DEV), fview, cview)


def ingest_yuv(left, right, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The 4:2:0 door on two YUVFrames of bytes."""
    from ppmstereo_amd.ppmstereo import byte_lut
    head = left.view_struct(), right.view_struct(), left.matrix()
    return ingest_door("yuv420", head, maps, left.n, (left.height, left.width), pad_left, pad_top, H, Wd, byte_lut(DEV), fview, cview)


def ingest_deep(left, right, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The generic YUV door on two YUVFrames of one format, with the level table of their depth."""
    from ppmstereo_amd.ppmstereo import level_lut
    fmt = left.format_struct()
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.sub_x, fmt.sub_y) == (right.sample_bytes, right.depth, right.lsb, right.sub_x, right.sub_y)
    lut = level_lut(DEV, left.depth)
    assert lut.numel() == 1 << left.depth
    head = left.view_struct(), right.view_struct(), left.matrix(), fmt
    return ingest_door("yuv", head, maps, left.n, (left.height, left.width), pad_left, pad_top, H, Wd, lut, fview, cview)


def ingest_raw(left, right, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The raw door on two RawFrames of one format, with the frames' own table."""
    assert left.same_format(right)
    lut = left.table(DEV)
    assert lut.numel() == 1 << left.depth and lut.is_cuda and lut.dtype == torch.float32
    head = left.view_struct(), right.view_struct(), left.format_struct()
    return ingest_door("raw", head, maps, left.n, (left.height, left.width), pad_left, pad_top, H, Wd, lut, fview, cview)


def ingest_packed(left, right, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The packed door of two PackedYUVFrames or two PackedRawFrames of one format."""
    from ppmstereo_amd.ppmstereo import PackedRawFrames, level_lut
    if isinstance(left, PackedRawFrames):
        assert left.same_format(right)
        entry, head, lut = "raw_packed", (left.view_struct(), right.view_struct(), left.format_struct()), left.table(DEV)
    else:
        assert (left.layout, left.lsb) == (right.layout, right.lsb)
        entry, head, lut = "yuv_packed", (left.view_struct(), right.view_struct(), left.matrix(), left.format_struct()), level_lut(DEV, left.depth)
    assert lut.numel() == 1 << left.depth
    return ingest_door(entry, head, maps, left.n, (left.height, left.width), pad_left, pad_top, H, Wd, lut, fview, cview)


def rotated_map(H0, W0, hs, ws, angle, scale, border, fill):
    """The rectified frame H0 x W0 as a rotated, scaled window around the centre of the hs x ws raw frame: its corners lie outside the raw frame."""
    import math

    from ppmstereo_amd.ppmstereo import RectifyMap
    ys, xs = torch.meshgrid(torch.arange(H0, dtype=torch.float32), torch.arange(W0, dtype=torch.float32), indexing="ij")
    dx, dy = xs - (W0 - 1) / 2, ys - (H0 - 1) / 2
    mx = (ws - 1) / 2 + scale * (math.cos(angle) * dx - math.sin(angle) * dy)
    my = (hs - 1) / 2 + scale * (math.sin(angle) * dx + math.cos(angle) * dy)
    m = RectifyMap.from_float(mx, my, (hs, ws), border, fill).to(DEV)
    x0, y0 = m.xy[..., 0], m.xy[..., 1]
    assert bool((x0 < 0).any()) and bool((x0 + 1 > ws - 1).any()) and bool((y0 < 0).any()) and bool((y0 + 1 > hs - 1).any())      # taps outside
    assert len(set(m.frac.reshape(-1).tolist())) > 500
    return m


@pytest.fixture(scope="module")
def model():
    """PPMStereo.shipped() with this package's encoders and the procedural weights (as tests/test_gpu_block.py builds the whole model)."""
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo
    from test_gpu_block import W
    m = PPMStereo.shipped()
    m.load_hot_path_weights(W)
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True)
    m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in ("disparity", "uncertainties"))
