"""CPU: the interleaved-RGB front door (BGR24 / RGB24, BGRA / RGBA / ARGB / ABGR, RGB48 / BGR48 / RGBA64 / BGRA64 at 10 and 12 bits, X2RGB10 /
X2BGR10).  The four ppms_video_*_rgb_packed entry points and the size export are declared, exported and bound as the header says; ``unpack()`` of
``PackedRGBFrames`` gives the levels that literal pixels written out by hand and this file's own packer (a pixel is a list of (value, bits) fields
summed into one Python integer) put there, whatever the alpha bytes, spare bits and pitch slack hold; ``from_hwc`` reads a tensor and a crop of it
where they lie; stereo_source dispatches without a device; and bad arguments are refused before any device is touched, by the plain entry and its
_remap twin with one message, and by the colour twins with the ingest door's message.  No device compute."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_colour_out as COLOUR
from colour_util import COLOUR_TAIL, ColourDoors, said
from ingest_util import (EINVAL, MAPS, TAIL, call_twin, ctype_of, header_args, lib, not_about_the_maps, one_message, packed_view,  # noqa: F401  (lib: the fixture)
                         sized_maps)

DOOR = "rgb_packed"
INGEST, INGEST_REMAP = "ppms_video_ingest_rgb_packed", "ppms_video_ingest_rgb_packed_remap"
HEAD = ["const ppms_packed_view* left", "const ppms_packed_view* right", "const ppms_rgb_packed_format* fmt"]
ENTRY_ARGS = {INGEST: HEAD + TAIL, INGEST_REMAP: HEAD + MAPS + TAIL,
              "ppms_video_colour_rgb_packed": HEAD + COLOUR_TAIL, "ppms_video_colour_rgb_packed_remap": HEAD + MAPS + COLOUR_TAIL}
SIZE_EXPORT = "ppms_rgb_packed_struct_size"

# layout: (container, components per pixel, the component -- for the 10-bit words the field -- that holds R, G, B), written out once more
LAYOUTS = {"rgb24": (0, 3, (0, 1, 2)), "bgr24": (0, 3, (2, 1, 0)), "rgba": (0, 4, (0, 1, 2)), "rgbx": (0, 4, (0, 1, 2)), "bgra": (0, 4, (2, 1, 0)),
           "bgrx": (0, 4, (2, 1, 0)), "argb": (0, 4, (1, 2, 3)), "xrgb": (0, 4, (1, 2, 3)), "abgr": (0, 4, (3, 2, 1)), "xbgr": (0, 4, (3, 2, 1)),
           "rgb48": (1, 3, (0, 1, 2)), "bgr48": (1, 3, (2, 1, 0)), "rgba64": (1, 4, (0, 1, 2)), "bgra64": (1, 4, (2, 1, 0)),
           "x2rgb10": (2, 1, (2, 1, 0)), "x2bgr10": (2, 1, (0, 1, 2))}
BYTE_LAYOUTS = [l for l, (c, _, _) in LAYOUTS.items() if c == 0]
# (layout, depth, align) of everything deeper than bytes
DEEP_FORMATS = [(l, d, a) for l, (c, _, _) in LAYOUTS.items() if c == 1 for d in (10, 12) for a in ("msb", "lsb")] + [("x2rgb10", 10, "msb"), ("x2bgr10", 10, "msb")]
FORMATS = [(l, 8, "msb") for l in BYTE_LAYOUTS] + DEEP_FORMATS


# ---- this file's packer: a pixel is a list of (value, bits) fields, lowest bit first, summed into one Python integer ----------------------------
def pixel_fields(layout, depth, align, rgb, junk):
    """rgb: the three levels of one pixel; junk(width): bits for what holds no level (alpha, spare bits of a word, bits 30 and 31)."""
    container, step, where = LAYOUTS[layout]
    slots = [None] * (3 if container == 2 else step)
    for level, at in zip(rgb, where):
        slots[at] = level
    if container == 2:
        return [(v, 10) for v in slots] + [(junk(2), 2)]
    fields = []
    for v in slots:
        v = junk(depth) if v is None else v                         # the fourth component
        if container == 0:
            fields.append((v, 8))
        else:
            spare = 16 - depth
            fields += [(junk(spare), spare), (v, depth)] if align == "msb" else [(v, depth), (junk(spare), spare)]
    return fields


def fields_to_bytes(fields):
    number, at = 0, 0
    for value, width in fields:
        assert 0 <= value < 2 ** width
        number += value * 2 ** at
        at += width
    assert at % 8 == 0
    return list(number.to_bytes(at // 8, "little"))


def packed_rgb(layout, depth, align, N, H, P, slack, seed, junk_seed=None, levels=None):
    """A random surface of P columns in `layout` with `slack` junk bytes behind every row: (the data tensor PackedRGBFrames takes -- uint8, uint16
    for words, int32 for the 10-bit words when the row allows --, the levels (N, 3, H, P) as int64).  junk_seed: other bits where no level lies."""
    container, step, _ = LAYOUTS[layout]
    rng = np.random.default_rng(seed + 7)
    S = rng.integers(0, 2 ** depth, (N, 3, H, P)) if levels is None else levels
    jr = np.random.default_rng(seed if junk_seed is None else junk_seed)
    junk = lambda width: int(jr.integers(0, 2 ** width))
    rows = [[[b for x in range(P) for b in fields_to_bytes(pixel_fields(layout, depth, align, S[n, :, y, x].tolist(), junk))] for y in range(H)] for n in range(N)]
    row_bytes = len(rows[0][0])
    assert row_bytes == (step * P, 2 * step * P, 4 * P)[container]
    out = jr.integers(0, 256, (N, H, row_bytes + slack), dtype=np.uint8)
    out[:, :, :row_bytes] = np.array(rows, dtype=np.uint8)
    data = torch.from_numpy(out)
    if container == 1:
        assert data.shape[2] % 2 == 0
        data = data.view(torch.uint16)                              # little-endian host
    return data, torch.from_numpy(S)


def planar(levels, depth):
    return levels.to(torch.uint8 if depth == 8 else torch.int16)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [*ENTRY_ARGS, SIZE_EXPORT])
def test_declared_exported_and_bound_as_the_header_says_and_abi_version_unchanged(lib, name):
    from ppmstereo_amd import _lib as L
    args = header_args(name)
    assert args == (ENTRY_ARGS[name] if name in ENTRY_ARGS else ["int* fmt"])
    assert name in L.EXPORTS and hasattr(lib, name) and lib.ppms_version() == 4

    def ctype(arg):
        special = {"const ppms_rgb_packed_format*": ctypes.POINTER(L.RGBPackedFormat), "const ppms_egress_plane*": ctypes.POINTER(L.EgressPlane)}
        kind = arg.rsplit(" ", 1)[0]
        return special[kind] if kind in special else ctype_of(arg)
    res, bound = L._SIGS[name]
    assert res is ctypes.c_int and bound == [ctype(a) for a in args]


def test_struct_size_fields_and_offsets(lib):
    from ppmstereo_amd import _lib as L
    size = ctypes.c_int()
    assert lib.ppms_rgb_packed_struct_size(ctypes.byref(size)) == 0 and size.value == ctypes.sizeof(L.RGBPackedFormat) == 32
    assert lib.ppms_rgb_packed_struct_size(None) == 0
    assert [n for n, _ in L.RGBPackedFormat._fields_] == ["container", "depth", "lsb", "step", "offset", "reserved"]
    assert {n: getattr(L.RGBPackedFormat, n).offset for n in ("container", "depth", "lsb", "step", "offset", "reserved")} == \
        dict(container=0, depth=4, lsb=8, step=12, offset=16, reserved=28)
    view, yuv, raw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()                 # the older packed structs are what they were
    assert lib.ppms_packed_struct_sizes(ctypes.byref(view), ctypes.byref(yuv), ctypes.byref(raw)) == 0 and (view.value, yuv.value, raw.value) == (24, 32, 48)


# ---- literal vectors: the layouts, written out by hand ------------------------------------------------------------------------------------------
def _rgb(frames):
    """[R, G, B] of the first pixel of the first row of the first frame."""
    return frames.unpack()[0, :, 0, 0].tolist()


def test_literal_byte_pixels():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames
    row = lambda *b: torch.tensor(b, dtype=torch.uint8).reshape(1, 1, -1)
    # bgr24: B = 10, G = 20, R = 30 in memory order; the same bytes read as rgb24 swap the ends
    assert _rgb(PackedRGBFrames(row(10, 20, 30), 1, "bgr24")) == [30, 20, 10] and _rgb(PackedRGBFrames(row(10, 20, 30), 1, "rgb24")) == [10, 20, 30]
    assert PackedRGBFrames(row(10, 20, 30), 1).layout == "bgr24"                  # the default: what OpenCV holds
    # argb: A = 200, R = 1, G = 2, B = 3; whatever the alpha byte holds
    for alpha in (200, 0, 255):
        px = row(alpha, 1, 2, 3)
        assert _rgb(PackedRGBFrames(px, 1, "argb")) == [1, 2, 3] and _rgb(PackedRGBFrames(px, 1, "xrgb")) == [1, 2, 3]
        assert _rgb(PackedRGBFrames(row(3, 2, 1, alpha), 1, "bgra")) == [1, 2, 3] and _rgb(PackedRGBFrames(row(1, 2, 3, alpha), 1, "rgbx")) == [1, 2, 3]
        assert _rgb(PackedRGBFrames(row(alpha, 3, 2, 1), 1, "abgr")) == [1, 2, 3]
    u = PackedRGBFrames(row(10, 20, 30, 40, 50, 60, 99, 98), 2, "bgr24").unpack()   # two pixels and two bytes of slack
    assert u.dtype == torch.uint8 and tuple(u.shape) == (1, 3, 1, 2) and u[0, :, 0].tolist() == [[30, 60], [20, 50], [10, 40]]
    assert PackedRGBFrames(row(10, 20, 30, 40, 50, 60, 99, 98), 1, "bgr24", x0=1).unpack()[0, :, 0, 0].tolist() == [60, 50, 40]


def test_literal_word_triples_at_both_alignments():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames
    words = lambda *w: torch.tensor(w, dtype=torch.int32).to(torch.uint16).reshape(1, 1, -1)
    # rgb48 at 10 bits, msb: R = 0x3A5, G = 0x001, B = 0x2AA in the top ten bits, garbage 0x3F, 0x15, 0x01 in the low six
    w = words(0xE97F, 0x0055, 0xAA81)
    top = PackedRGBFrames(w, 1, "rgb48", 10)
    assert _rgb(top) == [0x3A5, 0x001, 0x2AA] and top.unpack().dtype == torch.int16 and top.format_struct().lsb == 6
    assert _rgb(PackedRGBFrames(words(0xE940, 0x0040, 0xAA80), 1, "rgb48", 10)) == [0x3A5, 0x001, 0x2AA]      # the low bits dropped whatever they hold
    assert _rgb(PackedRGBFrames(w, 1, "bgr48", 10)) == [0x2AA, 0x001, 0x3A5]
    # the same words read from the bottom: the low ten bits, the high six masked
    low = PackedRGBFrames(w, 1, "rgb48", 10, "lsb")
    assert _rgb(low) == [0xE97F & 1023, 0x0055, 0xAA81 & 1023] == [0x17F, 0x055, 0x281] and low.format_struct().lsb == 0
    # 12 bits: msb takes the top twelve, lsb the low twelve
    assert _rgb(PackedRGBFrames(words(0xABCF, 0x1230, 0xFFF7), 1, "rgb48", 12)) == [0xABC, 0x123, 0xFFF]
    assert _rgb(PackedRGBFrames(words(0xFABC, 0x0123, 0x7FFF), 1, "rgb48", 12, "lsb")) == [0xABC, 0x123, 0xFFF]
    # a fourth word that is never read
    for alpha in (0, 0xFFFF):
        assert _rgb(PackedRGBFrames(words(0xFFC0, 0x8000, 0x0040, alpha), 1, "bgra64", 10)) == [0x001, 0x200, 0x3FF]


def test_literal_ten_bit_words_in_both_layouts():
    """0x3FF00000 is bits 29..20, 0x000FFC00 bits 19..10, 0x000003FF bits 9..0; bits 30 and 31 change nothing; bytes and int32 rows agree."""
    from ppmstereo_amd.ppmstereo import PackedRGBFrames
    for top in (0, 0x40000000, 0x80000000, 0xC0000000):
        for word, rgb10, bgr10 in ((0x3FF00000, [1023, 0, 0], [0, 0, 1023]), (0x000FFC00, [0, 1023, 0], [0, 1023, 0]), (0x000003FF, [0, 0, 1023], [1023, 0, 0]),
                                   (0x15500000 | 0x2AA << 10 | 0x0F0, [0x155, 0x2AA, 0x0F0], [0x0F0, 0x2AA, 0x155])):
            w = word | top
            as_bytes = torch.tensor([w & 255, (w >> 8) & 255, (w >> 16) & 255, (w >> 24) & 255], dtype=torch.uint8).reshape(1, 1, 4)
            as_int32 = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w], dtype=torch.int32).reshape(1, 1, 1)
            for data in (as_bytes, as_int32):
                assert _rgb(PackedRGBFrames(data, 1, "x2rgb10")) == rgb10 and _rgb(PackedRGBFrames(data, 1, "x2bgr10")) == bgr10, hex(w)
    f = PackedRGBFrames(as_int32, 1, "x2rgb10").format_struct()
    assert (f.container, f.depth, f.lsb, f.step, list(f.offset), f.reserved) == (2, 10, 0, 1, [2, 1, 0], 0)
    assert list(PackedRGBFrames(as_int32, 1, "x2bgr10").format_struct().offset) == [0, 1, 2]


# ---- unpack() gives the levels that were packed, whatever lies where no level lies --------------------------------------------------------------
@pytest.mark.parametrize("layout,depth,align", FORMATS, ids=[f"{l}-{d}-{a}" for l, d, a in FORMATS])
def test_unpack_equals_the_levels_that_were_packed_and_pack_round_trips(layout, depth, align):
    from ppmstereo_amd.ppmstereo import PackedRGBFrames
    container, step, where = LAYOUTS[layout]
    for width, x0 in ((50, 0), (37, 0), (50, 25), (37, 3)):
        P = x0 + width + 2
        data, S = packed_rgb(layout, depth, align, 2, 5, P, 8, 300 + width + x0)
        f = PackedRGBFrames(data, width, layout, depth, align, x0=x0)
        s, fmt, u = f.view_struct(), f.format_struct(), f.unpack()
        assert (s.data, s.pitch, s.frame_stride, s.x0) == (data.data_ptr(), data.stride(1) * data.element_size(), data.stride(0) * data.element_size(), x0)
        assert (fmt.container, fmt.depth, fmt.step, list(fmt.offset), fmt.reserved) == (container, depth, step, list(where), 0)
        assert fmt.lsb == (16 - depth if container == 1 and align == "msb" else 0)
        assert (f.n, f.height, f.width, f.depth) == (2, 5, width, depth) and u.dtype == (torch.uint8 if depth == 8 else torch.int16)
        assert torch.equal(u.long(), S[:, :, :, x0:x0 + width]), (layout, width, x0)
        assert torch.equal(f.to_rgb(), u) and torch.equal(f.to_float(), u.float() if depth == 8 else u.float() * (255.0 / (2 ** depth - 1)))
        # other bits in alpha, in the spare bits of words, in bits 30 and 31 and in the slack: the same levels
        other, _ = packed_rgb(layout, depth, align, 2, 5, P, 8, 300 + width + x0, junk_seed=900)
        assert not torch.equal(other, data) and torch.equal(PackedRGBFrames(other, width, layout, depth, align, x0=x0).unpack(), u)
        # unpack(pack(x)) == x, in dense rows whose unused bits are 0
        again = PackedRGBFrames.pack(u, layout, depth, align)
        assert (again.x0, again.width, again.layout, again.depth, again.lsb) == (0, width, layout, depth, f.lsb) and torch.equal(again.unpack(), u)
        assert again.data.shape[2] == again._row_elements(width) and again.data.is_contiguous()
        if container == 2:
            assert again.data.dtype == torch.int32 and not bool((again.data >> 30).any())
    if container == 2:                                                # the 10-bit words as int32 rows: the same bytes
        words = data[:, :, :4 * P].contiguous().view(torch.int32)
        assert torch.equal(PackedRGBFrames(words, width, layout, x0=x0).unpack(), u)
    for no_levels in (u.float(), u.long(), u[:, :2], u[0]) + (() if depth == 8 else (torch.full_like(u, 2 ** depth), torch.full_like(u, -1))):
        with pytest.raises(ValueError):
            PackedRGBFrames.pack(no_levels, layout, depth, align)


# ---- from_hwc: a tensor and a crop of it, where they lie ----------------------------------------------------------------------------------------
def test_from_hwc_reads_a_tensor_and_a_strided_crop_without_a_copy():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames, PackedRGBStereoVideo
    big = torch.randint(0, 256, (2, 45, 70, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(311))
    crop = big[:, 3:40, 5:55]
    assert not crop.is_contiguous()
    for order, pick in (("bgra", [2, 1, 0]), ("rgba", [0, 1, 2]), ("argb", [1, 2, 3]), ("xbgr", [3, 2, 1])):
        for t in (crop, crop.contiguous()):
            f = PackedRGBFrames.from_hwc(t, order)
            assert f.data.data_ptr() == t.data_ptr() and (f.n, f.height, f.width, f.x0, f.depth) == (2, 37, 50, 0, 8)
            assert (f.pitch, f.frame_stride) == (t.stride(1), t.stride(0)) and torch.equal(f.unpack(), t.permute(0, 3, 1, 2)[:, pick])
    three = torch.randint(0, 256, (2, 9, 11, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(312))
    assert PackedRGBFrames.from_hwc(three).layout == "bgr24" and torch.equal(PackedRGBFrames.from_hwc(three).unpack(), three.permute(0, 3, 1, 2)[:, [2, 1, 0]])
    assert torch.equal(PackedRGBFrames.from_hwc(three, "rgb").unpack(), three.permute(0, 3, 1, 2))
    words = torch.randint(0, 1 << 16, (2, 9, 11, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(313)).to(torch.uint16)
    w = PackedRGBFrames.from_hwc(words[:, 1:8, 2:9], "rgb", depth=12)
    assert (w.layout, w.depth, w.lsb, w.pitch, w.data.data_ptr()) == ("rgb48", 12, 4, 66, words[:, 1:8, 2:9].data_ptr())
    assert torch.equal(w.unpack().long(), words[:, 1:8, 2:9].permute(0, 3, 1, 2).to(torch.int32).long() >> 4)
    assert torch.equal(PackedRGBFrames.from_hwc(words, "bgr", 10, "lsb").unpack().long(), words.permute(0, 3, 1, 2)[:, [2, 1, 0]].to(torch.int32).long() & 1023)
    # what a copy to another device takes along: the view's own pixels, none of the tensor around the crop
    view = PackedRGBFrames.from_hwc(crop, "bgra")
    moved = view._moved("cpu")
    assert tuple(moved.data.shape) == (2, 37, 200) and (moved.x0, moved.width) == (0, 50) and torch.equal(moved.unpack(), view.unpack())
    # both views of one (N, 2, H, W, C) tensor
    video = torch.randint(0, 256, (3, 2, 8, 10, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(314))
    v = PackedRGBStereoVideo.from_hwc(video, "bgra")
    assert (len(v), v.height, v.width, v.depth) == (3, 8, 10, 8) and v.right.data.data_ptr() == video[:, 1].data_ptr() and v.left.frame_stride == 2 * 8 * 10 * 4
    assert torch.equal(v[1:].right.unpack(), video[1:, 1].permute(0, 3, 1, 2)[:, [2, 1, 0]]) and v.to("cpu").left is v.left
    for bad in (lambda: PackedRGBFrames.from_hwc(three, "bgra"), lambda: PackedRGBFrames.from_hwc(big, "bgr"), lambda: PackedRGBFrames.from_hwc(big, "gbr"),
                lambda: PackedRGBFrames.from_hwc(big.float(), "bgra"), lambda: PackedRGBFrames.from_hwc(big[0], "bgra"),
                lambda: PackedRGBFrames.from_hwc(big[:, :, ::2], "bgra"),          # a pixel stride of 8
                lambda: PackedRGBFrames.from_hwc(big.permute(0, 2, 1, 3), "bgra"),   # rows inside rows
                lambda: PackedRGBFrames.from_hwc(big[..., :3], "bgr"),             # three channels four bytes apart
                lambda: PackedRGBFrames.from_hwc(words, "rgb"),                    # words need a depth
                lambda: PackedRGBFrames.from_hwc(words, "rgb", 8), lambda: PackedRGBFrames.from_hwc(three, "rgb", 10),
                lambda: PackedRGBFrames.from_hwc(torch.zeros((2, 4, 4, 4), dtype=torch.uint16), "argb", 10),
                lambda: PackedRGBStereoVideo.from_hwc(big, "bgra"), lambda: PackedRGBStereoVideo.from_hwc(video[:, :1], "bgra")):
        with pytest.raises(ValueError):
            bad()


# ---- splits, slices and copies keep the surface -------------------------------------------------------------------------------------------------
def test_side_by_side_is_one_surface_with_two_x0():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames, PackedRGBStereoVideo
    data, S = packed_rgb("bgr24", 8, "msb", 3, 6, 100, 12, 441)
    p = PackedRGBFrames(data, 100)
    left, right = p.split_side_by_side()
    l, r = left.view_struct(), right.view_struct()
    assert (l.data, r.data, l.x0, r.x0, l.pitch, r.pitch, l.frame_stride, r.frame_stride) == (data.data_ptr(),) * 2 + (0, 50) + (312,) * 2 + (6 * 312,) * 2
    assert (right.width, right.height, right.layout) == (50, 6, "bgr24") and torch.equal(right.unpack().long(), S[:, :, :, 50:])
    video = PackedRGBStereoVideo(left, right)
    win = video[1:3]
    assert len(win) == 2 and win.right.view_struct().data == data.data_ptr() + 6 * 312 and win.right.x0 == 50
    assert torch.equal(win.right.to_rgb(), right.to_rgb()[1:3]) and video.to("cpu").left is left
    moved = right._moved("cpu")                                          # a copy holds the view's own pixels: x0 becomes 0
    assert (moved.x0, moved.width, moved.data.shape[2], moved.data.data_ptr() != data.data_ptr()) == (0, 50, 150, True) and torch.equal(moved.unpack(), right.unpack())
    odd_l, odd_r = PackedRGBFrames(data, 74, "bgr24", x0=3).split_side_by_side()  # halves of 37, inside a wider surface
    assert (odd_l.x0, odd_r.x0, odd_l.width, odd_r.width) == (3, 40, 37, 37) and torch.equal(odd_r.unpack().long(), S[:, :, :, 40:77])
    top, bottom = p.split_top_bottom()
    assert bottom.view_struct().data - top.view_struct().data == 3 * 312 and (bottom.height, bottom.width, bottom.x0) == (3, 100, 0)
    assert torch.equal(bottom.unpack().long(), S[:, :, 3:])
    xdata, X = packed_rgb("x2rgb10", 10, "msb", 2, 4, 30, 8, 442)
    a, b = PackedRGBFrames(xdata, 30, "x2rgb10").split_side_by_side()
    assert (b.x0, b.width, b.depth) == (15, 15, 10) and torch.equal(b.unpack().long(), X[:, :, :, 15:]) and b._moved("cpu").data.shape[2] == 60
    for bad in (lambda: PackedRGBFrames(data, 51).split_side_by_side(), lambda: PackedRGBFrames(data[:, :5], 50).split_top_bottom()):
        with pytest.raises(ValueError):
            bad()


def test_what_is_no_frame_raises():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames
    b = torch.zeros((2, 4, 64), dtype=torch.uint8)
    w = torch.zeros((2, 4, 64), dtype=torch.uint16)
    i = torch.zeros((2, 4, 16), dtype=torch.int32)
    PackedRGBFrames(b, 21), PackedRGBFrames(b, 16, "bgra"), PackedRGBFrames(w, 21, "rgb48", 10), PackedRGBFrames(w, 16, "bgra64", 12, "lsb")
    PackedRGBFrames(b, 16, "x2rgb10"), PackedRGBFrames(i, 16, "x2bgr10", 10), PackedRGBFrames(b, 16, "bgra", 8, "lsb"), PackedRGBFrames(b, 20, x0=1)
    PackedRGBFrames(b[:, :, 1:], 21)                                     # bytes at an odd address
    for bad in (lambda: PackedRGBFrames(b, 22),                           # 66 bytes needed
                lambda: PackedRGBFrames(b, 17, "rgba"), lambda: PackedRGBFrames(b, 17, "x2rgb10"), lambda: PackedRGBFrames(i, 17, "x2rgb10"),
                lambda: PackedRGBFrames(w, 17, "rgba64", 10), lambda: PackedRGBFrames(w, 22, "bgr48", 12),
                lambda: PackedRGBFrames(b, 16, "rgb565"), lambda: PackedRGBFrames(b, 16, "gbrp"), lambda: PackedRGBFrames(b, 16, align="top"),
                lambda: PackedRGBFrames(w, 16), lambda: PackedRGBFrames(b, 8, "rgb48", 10), lambda: PackedRGBFrames(i, 16, "bgra"),
                lambda: PackedRGBFrames(w, 16, "x2rgb10"), lambda: PackedRGBFrames(b.float(), 16),
                lambda: PackedRGBFrames(b, 16, depth=10), lambda: PackedRGBFrames(w, 16, "rgb48"), lambda: PackedRGBFrames(w, 16, "rgb48", 8),
                lambda: PackedRGBFrames(w, 16, "rgb48", 16), lambda: PackedRGBFrames(w, 16, "rgb48", 11), lambda: PackedRGBFrames(b, 16, "x2rgb10", 12),
                lambda: PackedRGBFrames(w, 16, "rgb48", 10, "top"),
                lambda: PackedRGBFrames(b, 20, x0=2), lambda: PackedRGBFrames(b, 20, x0=-1), lambda: PackedRGBFrames(b, 0), lambda: PackedRGBFrames(b[0], 16),
                lambda: PackedRGBFrames(b[:, :, 1:], 12, "x2rgb10"),       # an address that is no multiple of 4
                lambda: PackedRGBFrames(torch.zeros((2, 4, 66), dtype=torch.uint8), 16, "x2bgr10"),     # a pitch that is none
                lambda: PackedRGBFrames(b[:, :, ::2], 8),
                lambda: PackedRGBFrames(b.as_strided((2, 4, 64), (128, 32, 1)), 21),     # rows that overlap
                lambda: PackedRGBFrames(b.as_strided((2, 4, 64), (128, 64, 1)), 21)):    # frames that overlap
        with pytest.raises(ValueError):
            bad()


# ---- the front doors' argument checks -----------------------------------------------------------------------------------------------------------
def test_stereo_source_routes_interleaved_frames_without_a_device():
    from ppmstereo_amd.ppmstereo import PackedRGBFrames, PackedRGBStereoVideo, PackedYUVFrames, RectifyMap, StereoRectifier
    from ppmstereo_amd.video import _ByteSource, stereo_source
    hwc = torch.randint(0, 256, (2, 32, 128, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(451))
    left, right = PackedRGBFrames.from_hwc(hwc).split_side_by_side()
    src = stereo_source("PPMStereo.forward", left, right)
    assert isinstance(src, _ByteSource) and (src.n, src.b, src.size, src.depth, src._entry, src._maps) == (2, 1, (32, 64), 8, INGEST, ())
    frames = src._frames()
    assert len(frames) == 3 and (frames[0].data, frames[1].data, frames[0].x0, frames[1].x0) == (hwc.data_ptr(), hwc.data_ptr(), 0, 64)
    assert (frames[2].container, frames[2].depth, frames[2].step, list(frames[2].offset)) == (0, 8, 3, [2, 1, 0])
    assert src._planes()[0] is left.data and src.held()[1] is right.data
    fl, fr = src.float_views()
    assert torch.equal(fl, hwc[:, :, :64].permute(0, 3, 1, 2)[:, [2, 1, 0]].float()) and torch.equal(fr, right.to_float()) and tuple(fr.shape) == (2, 3, 32, 64)
    xdata, X = packed_rgb("x2rgb10", 10, "msb", 2, 32, 128, 0, 452)
    xl, xr = PackedRGBFrames(xdata, 128, "x2rgb10").split_side_by_side()
    deep = stereo_source("forward_batch_test", PackedRGBStereoVideo(xl, xr))
    assert (deep._entry, deep.depth, deep.size, deep.n) == (INGEST, 10, (32, 64), 2) and deep._frames()[2].container == 2
    assert torch.equal(deep.float_views()[1], X[:, :, :, 64:].float() * (255.0 / 1023))
    assert stereo_source("forward_batch_test", PackedRGBStereoVideo(xl, xr)[:1]).n == 1
    ident = RectifyMap(RectifyMap.identity(32, 64).xy, RectifyMap.identity(32, 64).frac, (32, 64), "constant", 255)
    rect = StereoRectifier(ident, ident)
    twin = stereo_source("forward_batch_test", PackedRGBStereoVideo(xl, xr), rectify=rect)
    assert twin._entry == INGEST_REMAP and [m.fill for m in twin._maps] == [1023, 1023]
    assert torch.equal(twin.float_views()[0], ident.apply_levels(xl.unpack(), 10).float() * (255.0 / 1023))
    assert stereo_source("PPMStereo.forward", left, right, rectify=rect)._maps[0].fill == 255
    with pytest.raises(ValueError):                                      # frames of another size than the maps' source
        stereo_source("PPMStereo.forward", left, right, rectify=StereoRectifier(RectifyMap.identity(30, 64), RectifyMap.identity(30, 64)))
    # mixed classes are no stereo pair
    yuyv = PackedYUVFrames(torch.zeros((2, 32, 128), dtype=torch.uint8), 64)
    for a, b in ((left, yuyv), (yuyv, right), (left, left.unpack()), (left.unpack(), right), (left, hwc), (hwc, right), (left, None)):
        with pytest.raises(TypeError):
            stereo_source("PPMStereo.forward", a, b)
    with pytest.raises(TypeError):
        PackedRGBStereoVideo(left, yuyv)
    # views that differ in layout, depth, alignment, size or frame count are none either
    four = torch.zeros((2, 32, 64, 4), dtype=torch.uint8)
    words = torch.zeros((2, 32, 64, 3), dtype=torch.uint16)
    w10 = PackedRGBFrames.from_hwc(words, "rgb", 10)
    for a, b in ((left, PackedRGBFrames(hwc.flatten(2), 64, "rgb24")), (left, PackedRGBFrames.from_hwc(four, "bgra")),
                 (PackedRGBFrames.from_hwc(four, "bgra"), PackedRGBFrames.from_hwc(four, "argb")), (w10, PackedRGBFrames.from_hwc(words, "rgb", 12)),
                 (w10, PackedRGBFrames.from_hwc(words, "rgb", 10, "lsb")), (w10, PackedRGBFrames.from_hwc(words, "bgr", 10)),
                 (xl, PackedRGBFrames(xdata, 64, "x2bgr10")), (left, PackedRGBFrames(hwc.flatten(2), 62)), (left, PackedRGBFrames(hwc.flatten(2)[:1], 64))):
        with pytest.raises(ValueError):
            stereo_source("PPMStereo.forward", a, b)
        with pytest.raises(ValueError):
            stereo_source("PPMStereo.forward", b, a)
    # bgra and bgrx are one way of reading, bytes and int32 rows of the 10-bit words too
    assert stereo_source("PPMStereo.forward", PackedRGBFrames.from_hwc(four, "bgra"), PackedRGBFrames.from_hwc(four, "bgrx")).depth == 8
    assert stereo_source("PPMStereo.forward", xl, PackedRGBFrames(xdata.view(torch.int32), 64, "x2rgb10", x0=64))._frames()[1].x0 == 64


# ---- argument refusal through the C ABI: frames of 37 x 50, two of them, padded to 64 x 64 ------------------------------------------------------
def rgb_call(lib, left=None, right=None, fmt=None, null=(), lmap=None, rmap=None, null_rmap=False, **geometry):
    """RGB48 frames of 10 bits at the top of their words (row: 6 * 50 = 300 bytes) in surfaces of pitch 320.  geometry: ingest_util.call's.
    lmap / rmap (dicts): the _remap twin."""
    from ppmstereo_amd import _lib as L
    f = dict(container=1, depth=10, lsb=6, step=3, offset=(0, 1, 2), reserved=0)
    f.update(fmt or {})
    view = functools.partial(packed_view, fs=37 * 320, pitch=320)
    head = [view(**(left or {})), view(**(right or {})), L.RGBPackedFormat(f["container"], f["depth"], f["lsb"], f["step"], f["offset"], f["reserved"])]
    return call_twin(lib, INGEST, head, null, lmap, rmap, null_rmap, **geometry)


OFF = dict(fnet=False, cnet=False)                                    # (a call that passes every check of its door gets as far as the destinations)
BGR24 = dict(container=0, depth=8, lsb=0, offset=(2, 1, 0))           # rows of 150 bytes
ARGB = dict(container=0, depth=8, lsb=0, step=4, offset=(1, 2, 3))    # rows of 200 bytes
X2 = dict(container=2, depth=10, lsb=0, step=1, offset=(2, 1, 0))     # rows of 200 bytes
# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [  # null pointers, non-zero reserved
    ("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(lut=0)),
    ("null data", dict(left=dict(data=0))), ("null data", dict(right=dict(data=0))),
    ("reserved", dict(fmt=dict(reserved=1))), ("reserved", dict(fmt=dict(X2, reserved=-1))),
    # container, depth, lsb, step: out of range, or not going together
    ("container", dict(fmt=dict(container=-1))), ("container", dict(fmt=dict(container=3))),
    ("depth", dict(fmt=dict(depth=8, lsb=0))), ("depth", dict(fmt=dict(depth=11, lsb=0))), ("depth", dict(fmt=dict(depth=16, lsb=0))),
    ("depth", dict(fmt=dict(BGR24, depth=10))), ("depth", dict(fmt=dict(X2, depth=12))), ("depth", dict(fmt=dict(X2, depth=8))),
    ("lsb", dict(fmt=dict(lsb=1))), ("lsb", dict(fmt=dict(lsb=4))), ("lsb", dict(fmt=dict(depth=12, lsb=6))), ("lsb", dict(fmt=dict(lsb=-6))),
    ("lsb", dict(fmt=dict(BGR24, lsb=8))), ("lsb", dict(fmt=dict(X2, lsb=6))),
    ("step", dict(fmt=dict(step=2))), ("step", dict(fmt=dict(step=5))), ("step", dict(fmt=dict(step=1))), ("step", dict(fmt=dict(step=0))),
    ("step", dict(fmt=dict(BGR24, step=1))), ("step", dict(fmt=dict(X2, step=3))), ("step", dict(fmt=dict(X2, step=4))),
    # offsets outside the pixel, and two channels in one place
    ("offset", dict(fmt=dict(offset=(0, 1, 3)))), ("offset", dict(fmt=dict(offset=(-1, 1, 2)))), ("offset", dict(fmt=dict(step=4, offset=(4, 1, 2)))),
    ("offset", dict(fmt=dict(BGR24, offset=(3, 2, 1)))), ("offset", dict(fmt=dict(X2, offset=(0, 1, 3)))), ("offset", dict(fmt=dict(X2, offset=(0, -1, 2)))),
    ("one place", dict(fmt=dict(offset=(0, 0, 1)))), ("one place", dict(fmt=dict(offset=(2, 1, 2)))), ("one place", dict(fmt=dict(ARGB, offset=(1, 3, 3)))),
    ("one place", dict(fmt=dict(X2, offset=(1, 1, 0)))),
    # x0
    ("x0", dict(left=dict(x0=-2))), ("x0", dict(right=dict(x0=-1))), ("65536", dict(right=dict(x0=65487, pitch=1 << 20, fs=37 << 20))),
    # 16-bit words at odd addresses, 32-bit words at addresses that are no multiple of 4
    ("misaligned", dict(left=dict(data=0x100001))), ("misaligned", dict(right=dict(pitch=319))), ("misaligned", dict(left=dict(fs=37 * 320 + 1))),
    ("multiples of 4", dict(fmt=X2, left=dict(data=0x100002))), ("multiples of 4", dict(fmt=X2, right=dict(pitch=318))),
    ("multiples of 4", dict(fmt=X2, right=dict(fs=37 * 320 + 2))),
    # rows and frames that overlap: 300 bytes a row, 306 from x0 = 1; bgr24 150; argb and the 10-bit words 200; rgba64 400
    ("pitch", dict(left=dict(pitch=298))), ("pitch", dict(right=dict(pitch=298))), ("pitch", dict(left=dict(x0=1, pitch=304, fs=37 * 304))),
    ("pitch", dict(fmt=BGR24, left=dict(pitch=149))), ("pitch", dict(fmt=ARGB, right=dict(pitch=199))), ("pitch", dict(fmt=X2, right=dict(pitch=196))),
    ("pitch", dict(fmt=X2, right=dict(x0=31, pitch=320))), ("pitch", dict(fmt=dict(step=4), left=dict(pitch=398, fs=37 * 398))),
    ("frame_stride", dict(left=dict(fs=36 * 320 + 298))), ("frame_stride", dict(right=dict(fs=0))), ("frame_stride", dict(fmt=BGR24, right=dict(fs=36 * 320 + 149))),
    # sizes, pads and destinations: video_ingest_launch's checks
    ("skipped", OFF), ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
    ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
    ("positive", dict(N=0)), ("positive", dict(H0=0)), ("positive", dict(W0=-2)),
    # (what is legal passes: a single frame needs no frame stride, bytes no alignment, the bounds themselves, every layout's exact row, any x0)
    ("skipped", dict(OFF, N=1, left=dict(fs=0), right=dict(fs=2))), ("skipped", dict(OFF, fmt=BGR24, left=dict(data=0x100001, pitch=151, fs=37 * 151))),
    ("skipped", dict(OFF, left=dict(pitch=300, fs=36 * 300 + 300), right=dict(x0=3, pitch=318))), ("skipped", dict(OFF, fmt=X2, left=dict(pitch=200, fs=37 * 200))),
    ("skipped", dict(OFF, fmt=dict(X2, offset=(0, 1, 2)), right=dict(x0=25, pitch=300))), ("skipped", dict(OFF, fmt=ARGB, left=dict(data=0x100003, pitch=201, fs=37 * 201))),
    ("skipped", dict(OFF, fmt=dict(step=4, offset=(2, 1, 3)), left=dict(pitch=400, fs=37 * 400), right=dict(pitch=400, fs=37 * 400))),
    ("skipped", dict(OFF, fmt=dict(depth=12, lsb=4))), ("skipped", dict(OFF, fmt=dict(lsb=0, offset=(2, 0, 1)))),
    ("skipped", dict(OFF, right=dict(x0=65486, pitch=1 << 20, fs=37 << 20))),
    # the _remap twin: what the other _remap calls refuse, a fill that is no level, and the door's checks against hs x ws
    ("null map", dict(null_rmap=True)), ("null xy", dict(lmap=dict(xy=0))), ("fill", dict(lmap=dict(fill=1024))), ("fill", dict(rmap=dict(fill=-1))),
    ("fill", dict(fmt=BGR24, lmap=dict(fill=256))), ("fill", dict(fmt=dict(depth=12, lsb=4), rmap=dict(fill=4096))), ("fill", dict(fmt=X2, rmap=dict(fill=1024))),
    ("pitch =", dict(lmap=dict(pitch=49))), ("border", dict(rmap=dict(border=2))), ("hs, ws", dict(rmap=dict(hs=36))),
    ("source frame", dict(lmap=dict(hs=0), rmap=dict(hs=0))), ("reserved", dict(rmap=dict(reserved=1))), ("misaligned", dict(lmap=dict(frac=0x500001))),
    ("depth", dict(lmap=dict(), fmt=dict(depth=9))), ("lsb", dict(rmap=dict(), fmt=dict(lsb=2))), ("misaligned pointer or stride", dict(lmap=dict(), left=dict(pitch=319))),
    ("container", dict(lmap=dict(), fmt=dict(container=5))), ("null", dict(rmap=dict(), null=(2,))), ("step", dict(rmap=dict(), fmt=dict(step=6))),
    ("one place", dict(lmap=dict(), fmt=dict(offset=(1, 1, 1)))), ("x0", dict(rmap=dict(), right=dict(x0=-7))),
    ("pitch", dict(lmap=dict(ws=65), rmap=dict(ws=65))),                                                  # 6 * 65 = 390 bytes a row
    ("frame_stride", dict(lmap=dict(hs=38), rmap=dict(hs=38))), ("65536", dict(lmap=dict(), left=dict(x0=65488, pitch=1 << 20, fs=37 << 20))),
    ("skipped", dict(OFF, lmap=dict(fill=1023))), ("skipped", dict(OFF, fmt=dict(depth=12, lsb=4), rmap=dict(fill=4095))), ("skipped", dict(OFF, fmt=BGR24, rmap=dict(fill=255))),
    ("skipped", dict(OFF, lmap=dict(hs=30, ws=53), rmap=dict(hs=30, ws=53)))]
IDS = [f"{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (_, b) in enumerate(BAD)]


@pytest.mark.parametrize("about,bad", BAD, ids=IDS)
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert rgb_call(lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_rgb_packed" in msg and about.encode() in msg, (bad, msg)
    assert (b"video_ingest_rgb_packed_remap" in msg) == ("lmap" in bad or "rmap" in bad or "null_rmap" in bad), msg


PARITY = [bad for _, bad in BAD if not_about_the_maps(bad)]


@pytest.mark.parametrize("bad", PARITY, ids=[f"{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, b in enumerate(PARITY)])
def test_plain_entry_and_remap_twin_refuse_with_one_message(lib, bad):
    """The rule of tests/test_ingest_doors.py (ingest_util.one_message), on this file's door."""
    one_message(lib, DOOR, rgb_call, lambda lib, **b: rgb_call(lib, **b, **sized_maps(b)), bad)


def test_destination_views_follow_img_s2d_contract(lib):
    from ppmstereo_amd import _lib as L
    v, f = packed_view(data=0x100001, fs=32 * 100, pitch=100), L.RGBPackedFormat(0, 8, 0, 3, (2, 1, 0), 0)
    go = lambda fd, cd: lib.ppms_video_ingest_rgb_packed(ctypes.byref(v), ctypes.byref(v), ctypes.byref(f), 1, 32, 32, 0, 0, 32, 32, 0x3000, fd, cd, None)
    for view in (L.SP(0x10000, None, 32, 32), L.SP(0x10000, 0x20000, 32, 8), L.SP(0x10000, 0x20000, 36, 32), L.SP(0x10008, 0x20000, 32, 32)):
        assert go(view, L.SP(None, None, 0, 0)) == EINVAL
        assert b"destination" in lib.ppms_last_error() and b"video_ingest_rgb_packed" in lib.ppms_last_error()


# ---- the colour twins ---------------------------------------------------------------------------------------------------------------------------
COLOUR_CALLS = (rgb_call, lambda lib, **kw: rgb_call(lib, lmap={}, rmap={}, **kw))        # (the twin: maps of the frames' own 37 x 50)


@pytest.mark.parametrize("about,changes,kw", COLOUR.COLOUR_BAD,
                         ids=[f"{a.replace(' ', '_')}:" + ",".join(f"{k}={v}" for k, v in {**c, **kw}.items()) for a, c, kw in COLOUR.COLOUR_BAD])
def test_colour_arguments_are_refused_with_one_message_by_the_door_and_its_twin(lib, about, changes, kw):
    """tests/test_colour_out.py's own table of what is wrong with a table, a plane, a frame range or a rectangle, on this door."""
    heard = []
    for entry in COLOUR_CALLS:
        lib.ppms_mem_attn_splits(3, 3, 256, 1)                  # (a successful call in between: the message below is this call's)
        heard.append(said(lib, entry(ColourDoors(lib, **changes), **kw)))
    (name, text), (twin_name, twin_text) = (m.split(": ", 1) for m in heard)
    assert name == "video_colour_rgb_packed" and twin_name == name + "_remap" and text == twin_text and about in text, heard


ONLY_INGEST = {"H", "W", "pad_left", "pad_top", "fnet", "cnet"}     # (what only the ingest launch checks; "skipped" calls would launch here)
COLOUR_DOOR_CASES = [bad for about, bad in BAD if about not in ("skipped", "null map") and not ONLY_INGEST & set(bad)]


@pytest.mark.parametrize("bad", COLOUR_DOOR_CASES, ids=[f"{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, b in enumerate(COLOUR_DOOR_CASES)])
def test_what_the_ingest_door_refuses_its_colour_twin_refuses_with_its_message(lib, bad):
    """Sources, formats and maps go through the ingest door's own checks.  The plane of these calls has reserved = 1, which the colour launch checks
    behind the door: a call the door lets through would end there, not in a launch."""
    lib.ppms_mem_attn_splits(3, 3, 256, 1)
    want = said(lib, rgb_call(lib, **bad))
    lib.ppms_mem_attn_splits(3, 3, 256, 1)
    got = said(lib, rgb_call(ColourDoors(lib, reserved=1), **bad))
    assert "out.reserved" not in got and got == want.replace("video_ingest_", "video_colour_"), (want, got)
