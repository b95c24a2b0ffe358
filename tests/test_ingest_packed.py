"""CPU: the packed front doors (YUYV / UYVY / YVYU / VYUY, Y210 / Y212, v210; MIPI CSI-2 RAW10 / RAW12 and PFNC 10p / 12p).  The four
ppms_video_ingest_*_packed entry points refuse bad arguments before touching a device, a plain entry and its _remap twin with one message (their
ABI: tests/test_ingest_doors.py); ``unpack()`` of the frame classes gives the
samples that were packed -- by this file's own packer, which writes every row as a list of (value, bits) fields into one Python integer, and by
literal vectors written out by hand; stereo_source dispatches packed frames without a device.  No device compute."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ingest_util import EINVAL, call_twin, lib, not_about_the_maps, one_message, packed_view, sized_maps  # noqa: F401  (lib: the fixture)

YUV, YUV_REMAP = "ppms_video_ingest_yuv_packed", "ppms_video_ingest_yuv_packed_remap"
RAW, RAW_REMAP = "ppms_video_ingest_raw_packed", "ppms_video_ingest_raw_packed_remap"
LAYOUTS = {"yuyv": (8, "YUYV"), "uyvy": (8, "UYVY"), "yvyu": (8, "YVYU"), "vyuy": (8, "VYUY"), "y210": (10, "YUYV"), "y212": (12, "YUYV"),
           "v210": (10, "UYVY")}                                       # layout: (depth, the four components of a pixel pair in memory order)
YUV_FORMATS = [(l, "msb") for l in LAYOUTS] + [("y210", "lsb"), ("y212", "lsb")]
RAW_FORMATS = [(p, d) for p in ("mipi", "pfnc") for d in (10, 12)]
PATTERNS = ["rggb", "bggr", "grbg", "gbrg", "mono"]


# ---- this file's packer: a row is a list of (value, bits) fields, lowest bit first, summed into one Python integer ------------------------------
def fields_to_bytes(fields):
    number, at = 0, 0
    for value, width in fields:
        assert 0 <= value < 2 ** width
        number += value * 2 ** at
        at += width
    assert at % 8 == 0
    return list(number.to_bytes(at // 8, "little"))


def yuv_row_fields(layout, align, ys, us, vs, junk):
    """ys: the luma of an even number of pixels, us / vs: the chroma of their pairs; junk(width): bits for what holds no sample."""
    depth, quad = LAYOUTS[layout]
    assert len(ys) % 2 == 0 and len(us) == len(vs) == len(ys) // 2
    comps = []
    for j in range(len(us)):
        luma = iter((ys[2 * j], ys[2 * j + 1]))
        comps += [next(luma) if k == "Y" else us[j] if k == "U" else vs[j] for k in quad]
    if layout == "v210":
        comps += [junk(10) for _ in range(-len(comps) % 12)]              # whole groups of 6 pixels
        return [f for w in range(len(comps) // 3) for f in ((comps[3 * w], 10), (comps[3 * w + 1], 10), (comps[3 * w + 2], 10), (junk(2), 2))]
    if depth == 8:
        return [(c, 8) for c in comps]
    spare = 16 - depth
    return [f for c in comps for f in (((junk(spare), spare), (c, depth)) if align == "msb" else ((c, depth), (junk(spare), spare)))]


def raw_row_fields(packing, depth, samples, junk):
    if packing == "pfnc":
        fields = [(s, depth) for s in samples]
        spare = -len(samples) * depth % 8
        return fields + ([(junk(spare), spare)] if spare else [])
    per, low = (4, 2) if depth == 10 else (2, 4)
    samples = list(samples) + [junk(depth) for _ in range(-len(samples) % per)]      # whole groups
    fields = []
    for g in range(len(samples) // per):
        group = samples[per * g:per * g + per]
        fields += [(s // 2 ** low, 8) for s in group] + [(s % 2 ** low, low) for s in group]
    return fields


def surface(rows_fields, N, H, slack, seed):
    """rows_fields(n, y, junk) -> the fields of one row; -> uint8 (N, H, row bytes + slack) whose slack bytes are random, and the row's bytes."""
    rng = np.random.default_rng(seed)
    junk = lambda width: int(rng.integers(0, 2 ** width))
    rows = [[fields_to_bytes(rows_fields(n, y, junk)) for y in range(H)] for n in range(N)]
    row_bytes = len(rows[0][0])
    out = rng.integers(0, 256, (N, H, row_bytes + slack), dtype=np.uint8)
    out[:, :, :row_bytes] = np.array(rows, dtype=np.uint8)
    return torch.from_numpy(out), row_bytes


def packed_yuv(layout, align, N, H, P, slack, seed, junk_seed=None):
    """A random surface of P columns (even) in `layout`: (PackedYUVFrames arguments' data, the samples Y (N, H, P), U, V (N, H, P / 2)).  junk_seed:
    other bits where no sample lies -- the spare bits of words, what follows the last pair inside a v210 group, the slack behind the row."""
    depth = LAYOUTS[layout][0]
    rng = np.random.default_rng(seed + 7)
    Y, U, V = rng.integers(0, 2 ** depth, (N, H, P)), rng.integers(0, 2 ** depth, (N, H, P // 2)), rng.integers(0, 2 ** depth, (N, H, P // 2))
    data, row_bytes = surface(lambda n, y, junk: yuv_row_fields(layout, align, Y[n, y].tolist(), U[n, y].tolist(), V[n, y].tolist(), junk), N, H, slack, seed if junk_seed is None else junk_seed)
    per = 2 if depth > 8 and layout != "v210" else 1
    assert row_bytes == (16 * -(-P // 6) if layout == "v210" else 4 * per * (P // 2))
    if per == 2:
        assert data.shape[2] % 2 == 0
        data = data.view(torch.uint16)                              # little-endian host
    return data, (Y, U, V)


def packed_raw(packing, depth, N, H, P, slack, seed, junk_seed=None):
    rng = np.random.default_rng(seed + 7)
    S = rng.integers(0, 2 ** depth, (N, H, P))
    data, row_bytes = surface(lambda n, y, junk: raw_row_fields(packing, depth, S[n, y].tolist(), junk), N, H, slack, seed if junk_seed is None else junk_seed)
    assert row_bytes == (-(-P * depth // 8) if packing == "pfnc" else 5 * -(-P // 4) if depth == 10 else 3 * -(-P // 2))
    return data, S


# ---- literal vectors: the layouts, written out by hand ---------------------------------------------------------------------------------------
def _le32(words):
    return torch.tensor([b for w in words for b in (w & 255, (w >> 8) & 255, (w >> 16) & 255, (w >> 24) & 255)], dtype=torch.uint8).reshape(1, 1, -1)


def test_literal_v210_group():
    """Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5, ten bits each from bit 0 up; bits 30 and 31 of words 1 and 3 are set and ignored."""
    from ppmstereo_amd.ppmstereo import PackedYUVFrames
    cb0, y0, cr0, y1, cb1, y2, cr1, y3, cb2, y4, cr2, y5 = 0x155, 0x2AA, 0x3FF, 0x001, 0x200, 0x0F0, 0x30C, 0x123, 0x3A5, 0x07E, 0x111, 0x2EF
    f = PackedYUVFrames(_le32([0x3FFAA955, 0xCF080001, 0x3A548F0C, 0xEEF4447E]), 6, "v210")
    u = f.unpack()
    assert (u.depth, u.chroma, u.y.dtype) == (10, "422", torch.uint16)
    assert u.y.tolist() == [[[y0, y1, y2, y3, y4, y5]]] and u.u.tolist() == [[[cb0, cb1, cb2]]] and u.v.tolist() == [[[cr0, cr1, cr2]]]
    assert PackedYUVFrames(f.data, 2, "v210", x0=2).unpack().y.tolist() == [[[y2, y3]]]            # a view that starts inside the group
    assert PackedYUVFrames(f.data, 2, "v210", x0=2).unpack().u.tolist() == [[[cb1]]]


def test_literal_mipi_and_pfnc_groups():
    from ppmstereo_amd.ppmstereo import PackedRawFrames
    raw = lambda bytes_, width, depth, packing: PackedRawFrames(torch.tensor(bytes_, dtype=torch.uint8).reshape(1, 1, -1), width, "mono", depth, packing)
    # RAW10: four top bytes, then the four pairs of low bits, pixel 0's lowest: 0x67 = 01 10 01 11
    assert raw([0xA9, 0x00, 0xFF, 0x55, 0x67], 4, 10, "mipi").unpack().data.tolist() == [[[0x2A7, 0x001, 0x3FE, 0x155]]]
    # RAW12: two top bytes, then the two low nibbles, pixel 0's lower
    assert raw([0xAB, 0x12, 0x3C], 2, 12, "mipi").unpack().data.tolist() == [[[0xABC, 0x123]]]
    # PFNC 10p: 0x2A7 | 0x001 << 10 | 0x3FE << 20 | 0x155 << 30 as five little-endian bytes; 12p: 0xABC | 0x123 << 12 as three
    assert raw([0xA7, 0x06, 0xE0, 0x7F, 0x55], 4, 10, "pfnc").unpack().data.tolist() == [[[0x2A7, 0x001, 0x3FE, 0x155]]]
    assert raw([0xBC, 0x3A, 0x12], 2, 12, "pfnc").unpack().data.tolist() == [[[0xABC, 0x123]]]
    assert raw([0xA7, 0x06, 0xE0, 0x7F, 0x55], 1, 10, "pfnc", ).unpack().data.tolist() == [[[0x2A7]]]
    assert PackedRawFrames(torch.tensor([0xA7, 0x06, 0xE0, 0x7F, 0x55], dtype=torch.uint8).reshape(1, 1, 5), 2, "mono", 10, "pfnc", x0=2).unpack().data.tolist() == \
        [[[0x3FE, 0x155]]]


def test_literal_byte_and_word_quads():
    from ppmstereo_amd.ppmstereo import PackedYUVFrames
    quad = torch.tensor([[[10, 20, 30, 40]]], dtype=torch.uint8)
    pick = lambda layout: [t.tolist()[0][0] for t in (lambda u: (u.y, u.u, u.v))(PackedYUVFrames(quad, 2, layout).unpack())]
    assert pick("yuyv") == [[10, 30], [20], [40]] and pick("uyvy") == [[20, 40], [10], [30]]
    assert pick("yvyu") == [[10, 30], [40], [20]] and pick("vyuy") == [[20, 40], [30], [10]]
    # Y210: Y0 = 0x3A5, U = 0x001, Y1 = 0x155, V = 0x2AA in the top ten bits, garbage 0x3F, 0x15, 0x2A, 0x01 in the low six
    words = torch.tensor([[[0xE97F, 0x0055, 0x556A, 0xAA81]]], dtype=torch.int32).to(torch.uint16)
    u = PackedYUVFrames(words, 2, "y210").unpack()
    assert (u.y.tolist(), u.u.tolist(), u.v.tolist()) == ([[[0x3A5, 0x155]]], [[[0x001]]], [[[0x2AA]]])
    low = PackedYUVFrames(words, 2, "y210", align="lsb").unpack()                # the same words read from the bottom: the low ten bits
    assert low.y.tolist() == [[[0xE97F & 1023, 0x556A & 1023]]]
    assert PackedYUVFrames(words, 2, "y210").format_struct().lsb == 6 and PackedYUVFrames(words, 2, "y210", align="lsb").format_struct().lsb == 0


# ---- unpack() gives the samples that were packed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,align", YUV_FORMATS)
def test_yuv_unpack_equals_the_samples_that_were_packed(layout, align):
    from ppmstereo_amd.ppmstereo import PackedYUVFrames, YUVFrames
    depth = LAYOUTS[layout][0]
    for width in (50, 37):
        for x0 in (0, 2, 26):
            P = x0 + width + (x0 + width) % 2
            data, (Y, U, V) = packed_yuv(layout, align, 2, 5, P, 8, 300 + width + x0)
            f = PackedYUVFrames(data, width, layout, align, x0=x0)
            s, fmt, u = f.view_struct(), f.format_struct(), f.unpack()
            assert (s.data, s.pitch, s.frame_stride, s.x0) == (data.data_ptr(), data.stride(1) * data.element_size(), data.stride(0) * data.element_size(), x0)
            assert (fmt.depth, list(fmt.reserved)) == (depth, [0, 0, 0, 0]) and fmt.lsb == (16 - depth if layout in ("y210", "y212") and align == "msb" else 0)
            assert (u.n, u.height, u.width, u.depth, u.chroma, u.lsb) == (2, 5, width, depth, "422", 0)
            wc = (width + 1) // 2
            assert torch.equal(u.y.long(), torch.from_numpy(Y[:, :, x0:x0 + width])), (layout, width, x0)
            assert torch.equal(u.u.long(), torch.from_numpy(U[:, :, x0 // 2:x0 // 2 + wc])) and torch.equal(u.v.long(), torch.from_numpy(V[:, :, x0 // 2:x0 // 2 + wc]))
            assert torch.equal(f.to_float(), u.to_float()) and torch.equal(f.to_rgb(), u.to_rgb())
            # pack(unpack(x)) keeps the payload: the same samples, in dense rows whose spare bits are 0
            again = PackedYUVFrames.pack(u, layout, align)
            assert (again.x0, again.width, again.layout, again.lsb) == (0, width, layout, f.lsb) and again.data.dtype == data.dtype
            v = again.unpack()
            assert torch.equal(v.y, u.y) and torch.equal(v.u, u.u) and torch.equal(v.v, u.v)
            if x0 == 0 and width % 2 == 0 and layout != "v210":
                spare = (1 << (16 - depth)) - 1 if depth > 8 else 0
                mask = 0xFFFF & ~(spare if align == "msb" else spare << depth) if depth > 8 else 0xFF
                assert torch.equal(again.data.long(), data[:, :, :again.data.shape[2]].long() & mask)
    if depth == 8:
        assert torch.equal(f.to_rgb_u8(), u.to_rgb_u8())
    else:
        with pytest.raises(ValueError):
            f.to_rgb_u8()


@pytest.mark.parametrize("packing,depth", RAW_FORMATS)
def test_raw_unpack_equals_the_samples_that_were_packed(packing, depth):
    from ppmstereo_amd.ppmstereo import PackedRawFrames
    for width in (50, 37):
        for x0 in (0, 1, 3, 25):
            data, S = packed_raw(packing, depth, 2, 5, x0 + width, 7, 400 + width + x0)
            f = PackedRawFrames(data, width, "gbrg", depth, packing, black=33, gains=(1.5, 1.0, 1.25), x0=x0)
            s, fmt, u = f.view_struct(), f.format_struct(), f.unpack()
            assert (s.data, s.pitch, s.frame_stride, s.x0) == (data.data_ptr(), data.shape[2], 5 * data.shape[2], x0)
            assert (fmt.packing, fmt.depth, fmt.pattern, fmt.black, list(fmt.gain), fmt.shift, list(fmt.reserved)) == \
                (int(packing == "pfnc"), depth, 3, 33, [1536, 1024, 1280], 10, [0, 0, 0, 0])
            assert (u.n, u.height, u.width, u.depth, u.pattern, u.lsb, u.black, u.gain_q) == (2, 5, width, depth, "gbrg", 0, 33, (1536, 1024, 1280))
            assert torch.equal(u.data.long(), torch.from_numpy(S[:, :, x0:x0 + width])), (packing, depth, width, x0)
            assert torch.equal(f.to_float(), u.to_float()) and torch.equal(f.to_rgb(), u.to_rgb())
            again = PackedRawFrames.pack(u, packing)
            assert (again.x0, again.width, again.packing, again.depth, again.pattern, again.black, again.gain_q) == (0, width, packing, depth, "gbrg", 33, f.gain_q)
            assert torch.equal(again.unpack().data, u.data)
            if x0 == 0:                                                # the payload's own bytes: every whole group of the row
                whole = (width // (4 if depth == 10 else 2)) * (5 if depth == 10 else 3)
                assert torch.equal(again.data[:, :, :whole], data[:, :, :whole])


def test_tone_curve_and_table_are_the_unpacked_frames():
    from ppmstereo_amd.ppmstereo import PackedRawFrames
    data, _ = packed_raw("mipi", 10, 2, 6, 12, 0, 431)
    tone = 255.0 * (torch.arange(1024, dtype=torch.float64) / 1023) ** (1 / 2.2)
    f = PackedRawFrames(data, 12, "rggb", 10, "mipi", tone=tone)
    assert f.tone.dtype == torch.float32 and torch.equal(f.to_float(), tone.float()[f.to_rgb().long()])
    assert f[1:].tone is f.tone and f.split_side_by_side()[1].tone is f.tone and f.unpack().tone is f.tone
    for bad in (tone[:-1], tone + 0.5, torch.arange(1024)):
        with pytest.raises(ValueError):
            PackedRawFrames(data, 12, "rggb", 10, "mipi", tone=bad)


def test_what_is_no_packed_frame_raises():
    from ppmstereo_amd.ppmstereo import PackedRawFrames, PackedYUVFrames
    b = torch.zeros((2, 4, 64), dtype=torch.uint8)
    w = torch.zeros((2, 4, 64), dtype=torch.uint16)
    PackedYUVFrames(b, 32), PackedYUVFrames(w, 16, "y212"), PackedYUVFrames(b, 24, "v210"), PackedRawFrames(b, 48), PackedRawFrames(b, 42, depth=12)
    PackedRawFrames(b, 51, packing="pfnc")
    PackedRawFrames(b[:, :1, :2], 1, "mono", 10, "pfnc")
    for bad in (lambda: PackedYUVFrames(b, 33),                         # 66 bytes needed
                lambda: PackedYUVFrames(b, 32, "nv12"), lambda: PackedYUVFrames(b, 32, align="top"), lambda: PackedYUVFrames(w, 16), lambda: PackedYUVFrames(b, 16, "y210"),
                lambda: PackedYUVFrames(b, 30, x0=3), lambda: PackedYUVFrames(b, 30, x0=-2), lambda: PackedYUVFrames(b, 0), lambda: PackedYUVFrames(b[0], 16),
                lambda: PackedYUVFrames(b, 25, "v210"),                  # 5 groups: 80 bytes
                lambda: PackedYUVFrames(b[:, :, 1:], 12, "v210"),        # an address that is no multiple of 4
                lambda: PackedYUVFrames(torch.zeros((2, 4, 66), dtype=torch.uint8), 24, "v210"),      # a pitch that is none
                lambda: PackedYUVFrames(b, 16, standard="bt2020"), lambda: PackedYUVFrames(b[:, :, ::2], 8),
                lambda: PackedRawFrames(b, 49), lambda: PackedRawFrames(b, 43, depth=12), lambda: PackedRawFrames(b, 52, packing="pfnc"),
                lambda: PackedRawFrames(b, 16, depth=8), lambda: PackedRawFrames(b, 16, depth=14), lambda: PackedRawFrames(b, 16, packing="csi"),
                lambda: PackedRawFrames(w, 16), lambda: PackedRawFrames(b, 16, "rgbg"), lambda: PackedRawFrames(b, 16, black=1024),
                lambda: PackedRawFrames(b, 16, gains=(1.0, 16.0, 1.0)), lambda: PackedRawFrames(b[:, :1], 16), lambda: PackedRawFrames(b, 1),
                lambda: PackedRawFrames(b.as_strided((2, 4, 64), (128, 32, 1)), 40)):       # rows that overlap
        with pytest.raises(ValueError):
            bad()


# ---- splits, slices and copies keep the surface -------------------------------------------------------------------------------------------------
def test_side_by_side_is_one_surface_with_two_x0():
    from ppmstereo_amd.ppmstereo import PackedRawFrames, PackedRawStereoVideo, PackedYUVFrames, PackedYUVStereoVideo
    data, (Y, U, V) = packed_yuv("v210", "msb", 3, 6, 100, 12, 441)               # halves of 50: the right one starts inside a group
    p = PackedYUVFrames(data, 100, "v210", standard="bt601", full_range=True)
    left, right = p.split_side_by_side()
    l, r = left.view_struct(), right.view_struct()
    assert (l.data, r.data, l.x0, r.x0, l.pitch, r.pitch, l.frame_stride, r.frame_stride) == (data.data_ptr(),) * 2 + (0, 50) + (data.shape[2],) * 2 + (6 * data.shape[2],) * 2
    assert (right.width, right.height, right.standard, right.full_range, right.layout) == (50, 6, "bt601", True, "v210")
    assert torch.equal(right.unpack().y.long(), torch.from_numpy(Y[:, :, 50:])) and torch.equal(right.unpack().v.long(), torch.from_numpy(V[:, :, 25:]))
    video = PackedYUVStereoVideo(left, right)
    assert (len(video), video.height, video.width, video.depth) == (3, 6, 50, 10)
    win = video[1:3]
    assert len(win) == 2 and win.right.view_struct().data == data.data_ptr() + 6 * data.shape[2] and win.right.x0 == 50
    assert torch.equal(win.right.to_rgb(), right.to_rgb()[1:3]) and video.to("cpu").left is left
    moved = right._moved("cpu")                                          # a copy holds the view's own groups: 48 = 8 * 6, so x0 becomes 2
    assert (moved.x0, moved.width, moved.data.shape[2], moved.data.data_ptr() != data.data_ptr()) == (2, 50, 16 * 17 - 16 * 8, True)
    assert torch.equal(moved.unpack().y, right.unpack().y) and torch.equal(moved.unpack().u, right.unpack().u)
    top, bottom = p.split_top_bottom()
    assert bottom.view_struct().data - top.view_struct().data == 3 * data.shape[2] and (bottom.height, bottom.width, bottom.x0) == (3, 100, 0)
    for bad in (lambda: PackedYUVFrames(data, 50, "v210").split_side_by_side(), lambda: PackedYUVFrames(data, 51, "v210").split_side_by_side(),
                lambda: PackedYUVFrames(data[:, :5], 50, "v210").split_top_bottom()):
        with pytest.raises(ValueError):
            bad()
    data, S = packed_raw("mipi", 10, 2, 8, 100, 5, 442)
    q = PackedRawFrames(data, 100, "grbg", 10, "mipi", black=64)
    a, b = q.split_side_by_side()
    assert (a.view_struct().data, b.view_struct().data, a.x0, b.x0, b.width, b.pattern, b.black) == (data.data_ptr(), data.data_ptr(), 0, 50, 50, "grbg", 64)
    assert torch.equal(b.unpack().data.long(), torch.from_numpy(S[:, :, 50:]))
    assert b._moved("cpu").x0 == 2 and torch.equal(b._moved("cpu").unpack().data, b.unpack().data)
    assert len(PackedRawStereoVideo(a, b)[1:]) == 1
    with pytest.raises(ValueError):
        PackedRawFrames(data, 50, "grbg").split_side_by_side()             # halves of 25: the right one would have another pattern
    m, n = PackedRawFrames(data, 50, "mono").split_side_by_side()
    assert (m.width, n.x0) == (25, 25)
    with pytest.raises(ValueError):
        PackedRawFrames(data[:, :6], 50, "grbg").split_top_bottom()


# ---- the front doors' argument checks --------------------------------------------------------------------------------------------------------
def test_stereo_source_routes_packed_frames_without_a_device():
    from ppmstereo_amd.ppmstereo import (PackedRawFrames, PackedRawStereoVideo, PackedYUVFrames, PackedYUVStereoVideo, RawFrames, RectifyMap, StereoRectifier,
                                         YUVFrames)
    from ppmstereo_amd.video import _ByteSource, stereo_source
    ydata, _ = packed_yuv("yuyv", "msb", 2, 32, 128, 0, 451)
    left, right = PackedYUVFrames(ydata, 128).split_side_by_side()
    src = stereo_source("PPMStereo.forward", left, right)
    assert isinstance(src, _ByteSource) and (src.n, src.b, src.size, src.depth, src._entry, src._maps) == (2, 1, (32, 64), 8, YUV, ())
    frames = src._frames()
    assert len(frames) == 4 and (frames[0].data, frames[1].data, frames[0].x0, frames[1].x0) == (ydata.data_ptr(), ydata.data_ptr(), 0, 64)
    assert (frames[3].container, frames[3].depth, frames[3].order) == (0, 8, 0) and frames[2].shift == 14
    assert src._planes()[0] is left.data and src.held()[1] is right.data
    fl, fr = src.float_views()
    assert torch.equal(fl, left.unpack().to_float()) and torch.equal(fr, right.to_float()) and tuple(fr.shape) == (2, 3, 32, 64)
    rdata, _ = packed_raw("pfnc", 12, 2, 32, 128, 0, 452)
    tone = 255.0 * (torch.arange(4096, dtype=torch.float32) / 4095) ** 0.45
    rl, rr = PackedRawFrames(rdata, 128, "bggr", 12, "pfnc", black=200, gains=(1.8, 1.0, 1.4), tone=tone).split_side_by_side()
    raw = stereo_source("forward_batch_test", PackedRawStereoVideo(rl, rr))
    assert (raw._entry, raw.depth, raw.size, raw.n) == (RAW, 12, (32, 64), 2) and len(raw._frames()) == 3 and raw._frames()[2].pattern == 1
    assert torch.equal(raw.float_views()[1], rr.unpack().to_float())
    assert stereo_source("forward_batch_test", PackedRawStereoVideo(rl, rr)[:1]).n == 1
    ident = RectifyMap(RectifyMap.identity(32, 64).xy, RectifyMap.identity(32, 64).frac, (32, 64), "constant", 255)
    rect = StereoRectifier(ident, ident)
    twin = stereo_source("forward_batch_test", PackedRawStereoVideo(rl, rr), rectify=rect)
    assert twin._entry == RAW_REMAP and [m.fill for m in twin._maps] == [4095, 4095]
    assert torch.equal(twin.float_views()[0], tone[ident.apply_levels(rl.to_rgb(), 12).long()])
    assert stereo_source("PPMStereo.forward", left, right, rectify=rect)._entry == YUV_REMAP
    assert stereo_source("forward_batch_test", PackedYUVStereoVideo(left, right), rectify=rect)._maps[0].fill == 255
    with pytest.raises(ValueError):                                      # frames of another size than the maps' source
        stereo_source("PPMStereo.forward", left, right, rectify=StereoRectifier(RectifyMap.identity(30, 64), RectifyMap.identity(30, 64)))
    # mixed classes are no stereo pair
    planar, unpacked = left.unpack(), rl.unpack()
    assert isinstance(planar, YUVFrames) and isinstance(unpacked, RawFrames)
    for a, b in ((left, rr), (rl, right), (left, planar), (planar, right), (rl, unpacked), (unpacked, rr), (left, ydata), (rdata, rr), (left, None)):
        with pytest.raises(TypeError):
            stereo_source("PPMStereo.forward", a, b)
    with pytest.raises(TypeError):
        PackedYUVStereoVideo(left, rr)
    # views that differ in layout, alignment, packing, depth, pattern or colour description are none either
    wdata, _ = packed_yuv("y210", "msb", 2, 32, 64, 0, 453)
    vdata, _ = packed_yuv("v210", "msb", 2, 32, 64, 0, 454)
    w210 = PackedYUVFrames(wdata, 64, "y210")
    for a, b in ((left, PackedYUVFrames(ydata, 64, "uyvy")), (left, PackedYUVFrames(ydata, 64, standard="bt601")), (left, PackedYUVFrames(ydata, 64, full_range=True)),
                 (w210, PackedYUVFrames(wdata, 64, "y210", align="lsb")), (w210, PackedYUVFrames(wdata, 64, "y212")), (w210, PackedYUVFrames(vdata, 64, "v210")),
                 (left, PackedYUVFrames(ydata, 62)), (left, PackedYUVFrames(ydata[:1], 64)),
                 (rl, PackedRawFrames(rdata, 64, "bggr", 12, "mipi", black=200, gains=(1.8, 1.0, 1.4), tone=tone)),
                 (rl, PackedRawFrames(rdata, 64, "rggb", 12, "pfnc", black=200, gains=(1.8, 1.0, 1.4), tone=tone)),
                 (rl, PackedRawFrames(rdata, 64, "bggr", 10, "pfnc", black=200, gains=(1.8, 1.0, 1.4))),
                 (rl, PackedRawFrames(rdata, 64, "bggr", 12, "pfnc", black=201, gains=(1.8, 1.0, 1.4), tone=tone)),
                 (rl, PackedRawFrames(rdata, 64, "bggr", 12, "pfnc", black=200, gains=(1.8, 1.0, 1.4)))):
        with pytest.raises(ValueError):
            stereo_source("PPMStereo.forward", a, b)
        with pytest.raises(ValueError):
            stereo_source("PPMStereo.forward", b, a)
    same = PackedRawFrames(rdata, 64, "bggr", 12, "pfnc", black=200, gains=(1.8, 1.0, 1.4), tone=tone.clone(), x0=64)      # an equal curve in another tensor
    assert stereo_source("PPMStereo.forward", rl, same)._frames()[1].x0 == 64


# ---- argument refusal through the C ABI: frames of 37 x 50, two of them, padded to 64 x 64 ------------------------------------------------------
def yuv_call(lib, left=None, right=None, fmt=None, mat=None, null=(), lmap=None, rmap=None, null_rmap=False, **geometry):
    """Y210 frames (row: 8 * 25 = 200 bytes) in surfaces of pitch 256.  geometry: ingest_util.call's.  lmap / rmap (dicts): the _remap twin."""
    from ppmstereo_amd import _lib as L
    f = dict(container=1, depth=10, lsb=6, order=0, reserved=(0, 0, 0, 0))
    f.update(fmt or {})
    m = dict(y_off=64, cy=19131, crv=29454, cgu=3504, cgv=8755, cbu=34707, shift=14, reserved=0)
    m.update(mat or {})
    head = [packed_view(**(left or {})), packed_view(**(right or {})), L.YUVMatrix(**m), L.YUVPackedFormat(f["container"], f["depth"], f["lsb"], f["order"], f["reserved"])]
    return call_twin(lib, YUV, head, null, lmap, rmap, null_rmap, **geometry)


def raw_call(lib, left=None, right=None, fmt=None, null=(), lmap=None, rmap=None, null_rmap=False, **geometry):
    """MIPI RAW10 frames (row: 5 * 13 = 65 bytes) in surfaces of pitch 80 at an odd address."""
    from ppmstereo_amd import _lib as L
    f = dict(packing=0, depth=10, pattern=0, black=64, gain=(1536, 1024, 1300), shift=10, reserved=(0, 0, 0, 0))
    f.update(fmt or {})
    view = functools.partial(packed_view, data=0x100001, fs=37 * 80, pitch=80)
    head = [view(**(left or {})), view(**(right or {})), L.RawPackedFormat(f["packing"], f["depth"], f["pattern"], f["black"], f["gain"], f["shift"], f["reserved"])]
    return call_twin(lib, RAW, head, null, lmap, rmap, null_rmap, **geometry)


OFF = dict(fnet=False, cnet=False)                                    # (a call that passes every check of its door gets as far as the destinations)
BYTES = dict(container=0, depth=8, lsb=0)                             # YUYV: rows of 100 bytes
V210 = dict(container=2, depth=10, lsb=0, order=1)                    # rows of 16 * 9 = 144 bytes
# (what the call's message must speak of, the one thing that is wrong with the call)
YUV_BAD = [  # null pointers, non-zero reserved
    ("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(null=(3,))), ("null", dict(lut=0)),
    ("null data", dict(left=dict(data=0))), ("null data", dict(right=dict(data=0))),
    ("reserved", dict(fmt=dict(reserved=(1, 0, 0, 0)))), ("reserved", dict(fmt=dict(reserved=(0, 0, 0, -1)))), ("reserved", dict(mat=dict(reserved=1))),
    # container, order, depth, lsb: out of range, or not going together
    ("container", dict(fmt=dict(container=-1))), ("container", dict(fmt=dict(container=3))),
    ("order", dict(fmt=dict(order=-1))), ("order", dict(fmt=dict(order=4))),
    ("depth", dict(fmt=dict(depth=8, lsb=0))), ("depth", dict(fmt=dict(depth=11, lsb=0))), ("depth", dict(fmt=dict(depth=16, lsb=0))),
    ("depth", dict(fmt=dict(BYTES, depth=10))), ("depth", dict(fmt=dict(V210, depth=12))), ("depth", dict(fmt=dict(V210, depth=8))),
    ("order = 0", dict(fmt=dict(V210, order=0))), ("order = 3", dict(fmt=dict(V210, order=3))),
    ("lsb", dict(fmt=dict(lsb=1))), ("lsb", dict(fmt=dict(lsb=4))), ("lsb", dict(fmt=dict(depth=12, lsb=6))), ("lsb", dict(fmt=dict(lsb=-6))),
    ("lsb", dict(fmt=dict(BYTES, lsb=8))), ("lsb", dict(fmt=dict(V210, lsb=6))),
    # x0
    ("x0", dict(left=dict(x0=-2))), ("x0", dict(right=dict(x0=-1))), ("even", dict(left=dict(x0=3))), ("even", dict(fmt=V210, right=dict(x0=1))),
    ("65536", dict(right=dict(x0=65488, pitch=1 << 20, fs=37 << 20))),
    # 16-bit words at odd addresses, v210 words at addresses that are no multiple of 4
    ("misaligned", dict(left=dict(data=0x100001))), ("misaligned", dict(right=dict(pitch=255))), ("misaligned", dict(left=dict(fs=37 * 256 + 1))),
    ("multiples of 4", dict(fmt=V210, left=dict(data=0x100002))), ("multiples of 4", dict(fmt=V210, right=dict(pitch=254))),
    ("multiples of 4", dict(fmt=V210, right=dict(fs=37 * 256 + 2))),
    # rows and frames that overlap: 200 bytes a row, 208 from x0 = 2; bytes 100; v210 144
    ("pitch", dict(left=dict(pitch=198))), ("pitch", dict(right=dict(pitch=198))), ("pitch", dict(left=dict(x0=2, pitch=204, fs=37 * 204))),
    ("pitch", dict(fmt=BYTES, left=dict(pitch=99))), ("pitch", dict(fmt=V210, right=dict(pitch=140))), ("pitch", dict(fmt=V210, right=dict(x0=6, pitch=144))),
    ("frame_stride", dict(left=dict(fs=36 * 256 + 198))), ("frame_stride", dict(right=dict(fs=0))), ("frame_stride", dict(fmt=BYTES, right=dict(fs=36 * 256 + 99))),
    # the matrix: ppms_video_ingest_yuv's bounds
    ("shift", dict(mat=dict(shift=7))), ("shift", dict(mat=dict(shift=17))), ("shift", dict(fmt=dict(depth=12, lsb=4), mat=dict(shift=15))),
    ("shift", dict(fmt=BYTES, mat=dict(shift=19))),
    ("y_off", dict(mat=dict(y_off=1024))), ("y_off", dict(mat=dict(y_off=-1))), ("y_off", dict(fmt=BYTES, mat=dict(y_off=256))),
    ("coefficient", dict(mat=dict(cy=-1))), ("coefficient", dict(mat=dict(crv=4 << 14))), ("coefficient", dict(mat=dict(cbu=4 << 14))),
    # sizes, pads and destinations: video_ingest_launch's checks
    ("skipped", OFF), ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
    ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
    ("positive", dict(N=0)), ("positive", dict(H0=0)), ("positive", dict(W0=-2)),
    # (what is legal passes: a single frame needs no frame stride, bytes no alignment, the bounds themselves, every layout's exact row)
    ("skipped", dict(OFF, N=1, left=dict(fs=0), right=dict(fs=2))), ("skipped", dict(OFF, fmt=BYTES, left=dict(data=0x100001, pitch=101, fs=37 * 101))),
    ("skipped", dict(OFF, left=dict(pitch=200, fs=36 * 200 + 200), right=dict(x0=2, pitch=208))), ("skipped", dict(OFF, fmt=V210, left=dict(pitch=144, fs=37 * 144))),
    ("skipped", dict(OFF, fmt=dict(V210), right=dict(x0=4, pitch=160))), ("skipped", dict(OFF, fmt=dict(lsb=0, order=3), mat=dict(shift=16, cy=(4 << 16) - 1))),
    ("skipped", dict(OFF, right=dict(x0=65486, pitch=1 << 20, fs=37 << 20))), ("skipped", dict(OFF, fmt=dict(depth=12, lsb=4), mat=dict(y_off=4095))),
    # the _remap twin: what the unpacked _remap calls refuse, a fill that is no level, and the door's checks against hs x ws
    ("null map", dict(null_rmap=True)), ("null xy", dict(lmap=dict(xy=0))), ("fill", dict(lmap=dict(fill=1024))), ("fill", dict(rmap=dict(fill=-1))),
    ("fill", dict(fmt=BYTES, lmap=dict(fill=256))), ("fill", dict(fmt=dict(depth=12, lsb=4), rmap=dict(fill=4096))),
    ("pitch =", dict(lmap=dict(pitch=49))), ("border", dict(rmap=dict(border=2))), ("hs, ws", dict(rmap=dict(hs=36))),
    ("source frame", dict(lmap=dict(hs=0), rmap=dict(hs=0))), ("reserved", dict(rmap=dict(reserved=1))), ("misaligned", dict(lmap=dict(frac=0x500001))),
    ("depth", dict(lmap=dict(), fmt=dict(depth=9))), ("lsb", dict(rmap=dict(), fmt=dict(lsb=2))), ("misaligned pointer or stride", dict(lmap=dict(), left=dict(pitch=255))),
    ("container", dict(lmap=dict(), fmt=dict(container=5))), ("null", dict(rmap=dict(), null=(3,))), ("even", dict(rmap=dict(), right=dict(x0=7))),
    ("pitch", dict(lmap=dict(ws=65), rmap=dict(ws=65))),                                                  # 8 * 33 = 264 bytes a row
    ("frame_stride", dict(lmap=dict(hs=38), rmap=dict(hs=38))), ("65536", dict(lmap=dict(), left=dict(x0=65488, pitch=1 << 20, fs=37 << 20))),
    ("skipped", dict(OFF, lmap=dict(fill=1023))), ("skipped", dict(OFF, fmt=dict(depth=12, lsb=4), rmap=dict(fill=4095))),
    ("skipped", dict(OFF, lmap=dict(hs=30, ws=64), rmap=dict(hs=30, ws=64)))]

MIPI12 = dict(depth=12)                                               # rows of 3 * 25 = 75 bytes
PFNC = dict(packing=1)                                                # rows of ceil(500 / 8) = 63 bytes; at depth 12 75
RAW_BAD = [  # null pointers, non-zero reserved
    ("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(lut=0)),
    ("null data", dict(left=dict(data=0))), ("null data", dict(right=dict(data=0))),
    ("reserved", dict(fmt=dict(reserved=(1, 0, 0, 0)))), ("reserved", dict(fmt=dict(reserved=(0, 0, 0, -1)))),
    # packing and depth
    ("packing", dict(fmt=dict(packing=-1))), ("packing", dict(fmt=dict(packing=2))),
    ("depth", dict(fmt=dict(depth=8))), ("depth", dict(fmt=dict(depth=11))), ("depth", dict(fmt=dict(depth=14))), ("depth", dict(fmt=dict(PFNC, depth=16))),
    # the mosaic, the black level, the white balance: ppms_video_ingest_raw's bounds
    ("pattern", dict(fmt=dict(pattern=-1))), ("pattern", dict(fmt=dict(pattern=5))),
    ("black", dict(fmt=dict(black=-1))), ("black", dict(fmt=dict(black=1024))), ("black", dict(fmt=dict(MIPI12, black=4096))),
    ("gain", dict(fmt=dict(gain=(-1, 1024, 1024)))), ("gain", dict(fmt=dict(gain=(1024, 16 << 10, 1024)))),
    ("gain", dict(fmt=dict(gain=(1024, 1024, 16 << 10)))), ("gain", dict(fmt=dict(gain=(16 << 4, 16, 16), shift=4))),
    ("shift", dict(fmt=dict(shift=3))), ("shift", dict(fmt=dict(shift=15))), ("shift", dict(fmt=dict(shift=-1))),
    # x0
    ("x0", dict(left=dict(x0=-1))), ("x0", dict(right=dict(x0=-3))), ("65536", dict(left=dict(x0=65487, pitch=1 << 20, fs=37 << 20))),
    # rows and frames that overlap: 65 bytes a row (70 from x0 = 3), RAW12 75, PFNC 63 / 75
    ("pitch", dict(left=dict(pitch=64))), ("pitch", dict(right=dict(pitch=64))), ("pitch", dict(right=dict(x0=3, pitch=69))),
    ("pitch", dict(fmt=MIPI12, left=dict(pitch=74))), ("pitch", dict(fmt=PFNC, left=dict(pitch=62))), ("pitch", dict(fmt=dict(PFNC, depth=12), right=dict(pitch=74))),
    ("pitch", dict(fmt=PFNC, left=dict(x0=1, pitch=63))),
    ("frame_stride", dict(left=dict(fs=36 * 80 + 64))), ("frame_stride", dict(right=dict(fs=0))), ("frame_stride", dict(fmt=PFNC, right=dict(fs=36 * 80 + 62))),
    # a colour pattern on a frame without neighbours
    ("2 x 2", dict(H0=1)), ("2 x 2", dict(W0=1)), ("2 x 2", dict(fmt=dict(pattern=3), H0=1, W0=1)),
    # sizes, pads and destinations: video_ingest_launch's checks
    ("skipped", OFF), ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
    ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
    ("positive", dict(N=0)), ("positive", dict(H0=0)), ("positive", dict(W0=-2)),
    # (what is legal passes: a single frame needs no frame stride, a monochrome frame no neighbours, any x0, the bounds and every packing's exact row)
    ("skipped", dict(OFF, N=1, left=dict(fs=0), right=dict(fs=2))), ("skipped", dict(OFF, fmt=dict(pattern=4), H0=1, W0=1)),
    ("skipped", dict(OFF, fmt=dict(black=1023, gain=(0, (16 << 10) - 1, 1)))), ("skipped", dict(OFF, fmt=dict(shift=14, gain=((16 << 14) - 1,) * 3))),
    ("skipped", dict(OFF, H0=2, W0=2)), ("skipped", dict(OFF, left=dict(pitch=65, fs=37 * 65), right=dict(x0=3, pitch=70, fs=37 * 70))),
    ("skipped", dict(OFF, fmt=MIPI12, left=dict(pitch=75, fs=36 * 75 + 75), right=dict(x0=1, pitch=78))),
    ("skipped", dict(OFF, fmt=PFNC, left=dict(pitch=63, fs=37 * 63), right=dict(x0=1, pitch=64))),
    ("skipped", dict(OFF, fmt=dict(PFNC, depth=12), left=dict(pitch=75), right=dict(x0=25, pitch=113, fs=37 * 113))),
    ("skipped", dict(OFF, left=dict(x0=65486, pitch=1 << 20, fs=37 << 20))),
    # the _remap twin
    ("null map", dict(null_rmap=True)), ("null xy", dict(lmap=dict(xy=0))), ("fill", dict(lmap=dict(fill=1024))), ("fill", dict(rmap=dict(fill=-1))),
    ("fill", dict(fmt=MIPI12, rmap=dict(fill=4096))),
    ("pitch =", dict(lmap=dict(pitch=49))), ("border", dict(rmap=dict(border=2))), ("hs, ws", dict(rmap=dict(hs=36))),
    ("source frame", dict(lmap=dict(hs=0), rmap=dict(hs=0))), ("reserved", dict(rmap=dict(reserved=1))), ("misaligned", dict(lmap=dict(frac=0x500001))),
    ("depth", dict(lmap=dict(), fmt=dict(depth=9))), ("packing", dict(rmap=dict(), fmt=dict(packing=3))), ("pattern", dict(lmap=dict(), fmt=dict(pattern=7))),
    ("null", dict(rmap=dict(), null=(2,))), ("x0", dict(lmap=dict(), right=dict(x0=-1))),
    ("pitch", dict(lmap=dict(ws=65), rmap=dict(ws=65))),                                                  # 5 * 17 = 85 bytes a row
    ("frame_stride", dict(lmap=dict(hs=38), rmap=dict(hs=38))), ("2 x 2", dict(lmap=dict(hs=1), rmap=dict(hs=1))),
    ("skipped", dict(OFF, lmap=dict(fill=1023))), ("skipped", dict(OFF, fmt=MIPI12, rmap=dict(fill=4095))),
    ("skipped", dict(OFF, lmap=dict(hs=30, ws=64), rmap=dict(hs=30, ws=64)))]

DOORS = {"yuv_packed": (yuv_call, YUV_BAD), "raw_packed": (raw_call, RAW_BAD)}
CASES = [(door, about, bad) for door, (_, cases) in DOORS.items() for about, bad in cases]


@pytest.mark.parametrize("door,about,bad", CASES, ids=[f"{d}:{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (d, _, b) in enumerate(CASES)])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, door, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert DOORS[door][0](lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_" + door.encode() in msg and about.encode() in msg, (bad, msg)
    assert (b"video_ingest_" + door.encode() + b"_remap" in msg) == ("lmap" in bad or "rmap" in bad or "null_rmap" in bad), msg


PARITY = [(door, bad) for door, _, bad in CASES if not_about_the_maps(bad)]


@pytest.mark.parametrize("door,bad", PARITY, ids=[f"{d}:{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (d, b) in enumerate(PARITY)])
def test_plain_entry_and_remap_twin_refuse_with_one_message(lib, door, bad):
    """The rule of tests/test_ingest_doors.py (ingest_util.one_message), on this file's two doors."""
    entry = DOORS[door][0]
    one_message(lib, door, entry, lambda lib, **b: entry(lib, **b, **sized_maps(b)), bad)


def test_destination_views_follow_img_s2d_contract(lib):
    from ppmstereo_amd import _lib as L
    v, f = packed_view(data=0x100001, fs=32 * 40, pitch=40), L.RawPackedFormat(1, 10, 1, 0, (1024, 1024, 1024), 10, (0, 0, 0, 0))
    go = lambda fd, cd: lib.ppms_video_ingest_raw_packed(ctypes.byref(v), ctypes.byref(v), ctypes.byref(f), 1, 32, 32, 0, 0, 32, 32, 0x3000, fd, cd, None)
    for view in (L.SP(0x10000, None, 32, 32), L.SP(0x10000, 0x20000, 32, 8), L.SP(0x10000, 0x20000, 36, 32), L.SP(0x10008, 0x20000, 32, 32)):
        assert go(view, L.SP(None, None, 0, 0)) == EINVAL
        assert b"destination" in lib.ppms_last_error() and b"video_ingest_raw_packed" in lib.ppms_last_error()
