"""CPU: the decoded-video front door for 10- / 12-bit samples and 4:2:2 / 4:4:4 chroma.  ppms_video_ingest_yuv and its _remap twin refuse bad
arguments before touching a device (their ABI: tests/test_ingest_doors.py); yuv_matrix(depth=)
/ YUVFrames.to_rgb are the conversion the header states (against float64), YUVFrames reads byte strides, alignment and subsampling from views
without copying, and RectifyMap.apply_levels / level_fill are the remap on levels.  No device compute."""
import ctypes
import functools
import itertools

import pytest
import torch

from ingest_util import EINVAL, call_twin, lib, rand_u8, rand_u16, remap_view, yuv_view  # noqa: F401  (lib: the fixture)
from test_ingest_yuv import COMBOS, STANDARDS

NAME, REMAP = "ppms_video_ingest_yuv", "ppms_video_ingest_yuv_remap"


# ---- argument refusal: P010 frames of 37 x 50 (chroma 19 x 25 pairs) in surfaces of pitch 128 bytes, two frames, padded to 64 x 64 -----------
_view = functools.partial(yuv_view, y=0x100000, u=0x200000, v=0x200002, fsy=37 * 128, fsc=19 * 128, pitch_y=128, pitch_c=128, step_c=4)
_map = functools.partial(remap_view, border=1)


def _call(lib, left=None, right=None, fmt=None, null=(), lmap=None, rmap=None, **kw):
    """kw: fields of the matrix, and the call's geometry (ingest_util.call).  lmap / rmap (dicts): the _remap twin."""
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import yuv_matrix
    f = dict(sample_bytes=2, depth=10, lsb=6, sub_x=1, sub_y=1, reserved=(0, 0, 0))
    f.update(fmt or {})
    mat = yuv_matrix(depth=f["depth"] if f["depth"] in (8, 10, 12) else 10)
    for k in [k for k in kw if hasattr(mat, k)]:
        setattr(mat, k, kw.pop(k))
    head = [_view(**(left or {})), _view(**(right or {})), mat, L.YUVFormat(f["sample_bytes"], f["depth"], f["lsb"], f["sub_x"], f["sub_y"], f["reserved"])]
    return call_twin(lib, NAME, head, null, lmap, rmap, **kw)


BYTES = dict(sample_bytes=1, depth=8, lsb=0)                          # (with the P010 views' strides, which are large enough for bytes too)
# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [  # every case the 4:2:0 call refuses
       ("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(null=(3,))), ("null", dict(lut=0)),
       ("null plane", dict(left=dict(y=0))), ("null plane", dict(right=dict(u=0))), ("null plane", dict(left=dict(v=0))),
       ("step_c", dict(left=dict(step_c=0))), ("step_c", dict(right=dict(step_c=1))), ("step_c", dict(right=dict(step_c=8))),
       ("step_c", dict(fmt=BYTES, left=dict(step_c=4))),
       ("pitch_y", dict(left=dict(pitch_y=98))), ("pitch_y", dict(right=dict(pitch_y=98))),                              # < 2 * 50 bytes
       ("pitch_c", dict(left=dict(pitch_c=96))), ("pitch_c", dict(right=dict(pitch_c=48, step_c=2))),                    # < 4 * 24 + 2, < 2 * 24 + 2
       ("frame_stride_y", dict(left=dict(fsy=36 * 128 + 98))), ("frame_stride_c", dict(right=dict(fsc=18 * 128 + 96))),  # frames overlap
       ("shift", dict(shift=7)), ("shift", dict(shift=17)), ("shift", dict(fmt=dict(depth=12, lsb=4), shift=15)),        # [8, 26 - depth]
       ("shift", dict(fmt=BYTES, left=dict(step_c=2), right=dict(step_c=2), shift=19)),
       ("reserved", dict(left=dict(reserved=1))), ("reserved", dict(right=dict(reserved=-1))), ("reserved", dict(reserved=1)),
       ("skipped", dict(fnet=False, cnet=False)),
       ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
       ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
       ("positive", dict(N=0)), ("positive", dict(H0=0)),
       ("coefficient", dict(cy=-1)), ("coefficient", dict(crv=4 << 14)),
       # the format
       ("sample_bytes", dict(fmt=dict(sample_bytes=0))), ("sample_bytes", dict(fmt=dict(sample_bytes=3))), ("sample_bytes", dict(fmt=dict(sample_bytes=4))),
       ("depth", dict(fmt=dict(sample_bytes=1, depth=10, lsb=0))), ("depth", dict(fmt=dict(depth=8, lsb=0))), ("depth", dict(fmt=dict(depth=11, lsb=0))),
       ("depth", dict(fmt=dict(depth=16, lsb=0))), ("depth", dict(fmt=dict(sample_bytes=1, depth=12, lsb=0))),
       ("lsb", dict(fmt=dict(lsb=1))), ("lsb", dict(fmt=dict(lsb=4))), ("lsb", dict(fmt=dict(depth=12, lsb=6))), ("lsb", dict(fmt=dict(lsb=-6))),
       ("lsb", dict(fmt=dict(sample_bytes=1, depth=8, lsb=8))),
       ("sub_x", dict(fmt=dict(sub_x=0, sub_y=1))), ("sub_x", dict(fmt=dict(sub_x=2, sub_y=1))), ("sub_x", dict(fmt=dict(sub_x=1, sub_y=2))),
       ("sub_x", dict(fmt=dict(sub_x=-1, sub_y=0))),
       ("reserved", dict(fmt=dict(reserved=(1, 0, 0)))), ("reserved", dict(fmt=dict(reserved=(0, 0, -1)))),
       # 16-bit samples at odd addresses
       ("odd", dict(left=dict(y=0x100001))), ("odd", dict(right=dict(u=0x200001))), ("odd", dict(left=dict(v=0x200003))),
       ("odd", dict(left=dict(pitch_y=129))), ("odd", dict(right=dict(pitch_c=127))), ("odd", dict(left=dict(fsy=37 * 128 + 1))),
       ("odd", dict(right=dict(fsc=19 * 128 + 1))),
       # strides too small for the subsampling: 4:2:2 has 37 chroma rows, 4:4:4 rows of 50 pairs
       ("frame_stride_c", dict(fmt=dict(sub_y=0))), ("pitch_c", dict(fmt=dict(sub_x=0, sub_y=0), left=dict(fsc=37 * 128), right=dict(fsc=37 * 128))),
       ("y_off", dict(y_off=1024)), ("y_off", dict(y_off=-1)), ("y_off", dict(fmt=BYTES, left=dict(step_c=2), right=dict(step_c=2), y_off=256)),
       # the _remap twin: what the twin of the 4:2:0 call refuses, and a fill that is no level
       ("null map", dict(lmap=dict(), rmap=None, null=())), ("fill", dict(lmap=dict(fill=1024))), ("fill", dict(rmap=dict(fill=-1))),
       ("fill", dict(fmt=BYTES, left=dict(step_c=2), right=dict(step_c=2), lmap=dict(fill=256))),
       ("fill", dict(fmt=dict(depth=12, lsb=4), rmap=dict(fill=4096))),
       ("pitch =", dict(lmap=dict(pitch=49))), ("border", dict(rmap=dict(border=2))), ("hs, ws", dict(rmap=dict(hs=36))),
       ("depth", dict(lmap=dict(), fmt=dict(depth=9))), ("lsb", dict(rmap=dict(), fmt=dict(lsb=2))), ("odd", dict(lmap=dict(), left=dict(pitch_c=127))),
       # (a fill that IS a level passes the check: the call gets as far as the destinations)
       ("skipped", dict(lmap=dict(fill=1023), fnet=False, cnet=False)),
       ("skipped", dict(fmt=dict(depth=12, lsb=4), rmap=dict(fill=4095), fnet=False, cnet=False))]


def _null_map_call(lib):
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import yuv_matrix
    v, m, f, mp = _view(), yuv_matrix(depth=10), L.YUVFormat(2, 10, 6, 1, 1, (0, 0, 0)), _map()
    sp = L.SP(0x10000, 0x20000, 32, 32)
    return lib.ppms_video_ingest_yuv_remap(ctypes.byref(v), ctypes.byref(v), ctypes.byref(m), ctypes.byref(f), ctypes.byref(mp), None, 2, 37, 50, 7, 13, 64, 64,
                                           0x3000, sp, L.SP(None, None, 0, 0), None)


@pytest.mark.parametrize("about,bad", BAD, ids=[f"{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (_, b) in enumerate(BAD)])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    rc = _null_map_call(lib) if about == "null map" else _call(lib, **bad)
    assert rc == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_yuv" in msg and b"yuv420" not in msg and about.encode() in msg, (bad, msg)
    assert (b"video_ingest_yuv_remap" in msg) == ("lmap" in bad or "rmap" in bad or about == "null map"), msg


# ---- the conversion ------------------------------------------------------------------------------------------------------------------
def float64_levels(y, u, v, standard, full_range, depth):
    """The YCbCr -> RGB equations in float64 on `depth`-bit samples, rounded half up and clamped (y, u, v: int64 tensors) -> (3, ...) int64."""
    kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    top, up = 2 ** depth - 1, 2 ** (depth - 8)
    sy, sc, off = (1.0, 1.0, 0) if full_range else (top / (219.0 * up), top / (224.0 * up), 16 * up)
    d, e, f = (y - off).double() * sy, (u - 128 * up).double() * sc, (v - 128 * up).double() * sc
    r = d + 2.0 * (1.0 - kr) * f
    g = d - 2.0 * kb * (1.0 - kb) / kg * e - 2.0 * kr * (1.0 - kr) / kg * f
    b = d + 2.0 * (1.0 - kb) * e
    return torch.floor(torch.stack([r, g, b]) + 0.5).clamp(0, top).long()


def one_pixel_frames(y, u, v, standard, full_range, depth, align="lsb", chroma="444"):
    """Every (Y, U, V) triple as a frame of one pixel."""
    from ppmstereo_amd.ppmstereo import YUVFrames
    as_plane = lambda t: t.to(torch.int32).to(torch.uint8 if depth == 8 else torch.uint16).reshape(-1, 1, 1)
    return YUVFrames.planar(as_plane(y), as_plane(u), as_plane(v), depth=depth, chroma=chroma, align=align, standard=standard, full_range=full_range)


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("standard,full_range", COMBOS)
def test_to_rgb_against_float64(standard, full_range, depth):
    """A 9-step grid of (Y, U, V) plus the corners.  At shift = 14 three coefficients, each off by at most 2^-15, times operands of at most 4095
    move a sum by less than 0.38 level: only ties and their neighbours can differ from the float64 result, by one level."""
    from ppmstereo_amd.ppmstereo import yuv_matrix
    top = 2 ** depth - 1
    levels = torch.tensor(sorted(set(range(0, top + 1, (top + 1) // 8)) | {top}))
    y, u, v = (t.reshape(-1) for t in torch.meshgrid(levels, levels, levels, indexing="ij"))
    assert {(0, 0, 0), (top, top, top), (0, top, 0), (top, 0, top)} <= set(zip(y.tolist(), u.tolist(), v.tolist()))
    got = one_pixel_frames(y, u, v, standard, full_range, depth).to_rgb()
    assert got.dtype == torch.int16 and tuple(got.shape) == (y.numel(), 3, 1, 1)
    want = float64_levels(y, u, v, standard, full_range, depth)
    diff = (got.reshape(-1, 3).long().T - want).abs()
    assert int(diff.max()) <= 1, int(diff.max())
    assert int(got.min()) == 0 and int(got.max()) == top
    m = yuv_matrix(standard, full_range, depth=depth)
    up = 2 ** (depth - 8)
    assert (m.shift, m.reserved, m.y_off) == (14, 0, 0 if full_range else 16 * up)
    kr, kb = STANDARDS[standard]
    sc = 1.0 if full_range else top / (224.0 * up)
    assert m.crv == round(sc * 2 * (1 - kr) * 16384) and m.cbu == round(sc * 2 * (1 - kb) * 16384)
    assert m.cy == (16384 if full_range else round(top / (219.0 * up) * 16384))


@pytest.mark.parametrize("standard", ["bt709", "bt601"])
def test_grey_axis(standard):
    for depth, (lo, hi) in ((10, (64, 940)), (12, (256, 3760))):
        n, top = 2 ** depth, 2 ** depth - 1
        grey = torch.full((n,), n // 2)
        full = one_pixel_frames(torch.arange(n), grey, grey, standard, True, depth).to_rgb().reshape(n, 3)
        assert torch.equal(full, torch.arange(n, dtype=torch.int16)[:, None].expand(n, 3))                 # full range: the identity on all levels
        lim = one_pixel_frames(torch.tensor([lo, hi, 0, top]), grey[:4], grey[:4], standard, False, depth).to_rgb().reshape(4, 3)
        assert lim.tolist() == [[0, 0, 0], [top, top, top], [0, 0, 0], [top, top, top]]


def test_depth_8_is_what_it_was():
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import YUVFrames, yuv_matrix
    names = [n for n, _ in L.YUVMatrix._fields_]
    for (standard, full_range), shift in itertools.product(COMBOS, (8, 14, 20)):
        a, b = yuv_matrix(standard, full_range, shift), yuv_matrix(standard, full_range, shift, depth=8)
        assert [getattr(a, n) for n in names] == [getattr(b, n) for n in names]
    for kw in (dict(depth=9), dict(depth=16), dict(depth=10, shift=17), dict(depth=12, shift=15), dict(depth=10, standard="bt2020")):
        with pytest.raises(ValueError):
            yuv_matrix(**kw)
    assert yuv_matrix(depth=10, shift=16).shift == 16 and yuv_matrix(depth=12, shift=14).y_off == 256
    f = YUVFrames.nv12(rand_u8((2, 37, 51), 1), rand_u8((2, 19, 26, 2), 2), "bt601", True)
    assert (f.depth, f.chroma, f.lsb, f.sample_bytes) == (8, "420", 0, 1)
    rgb = f.to_rgb()
    assert rgb.dtype == torch.uint8 and torch.equal(rgb, f.to_rgb_u8())
    assert torch.equal(f.to_float(), rgb.float()) and f.to_float().dtype == torch.float32
    fmt = f.format_struct()
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.sub_x, fmt.sub_y, list(fmt.reserved)) == (1, 8, 0, 1, 1, [0, 0, 0])
    assert YUVFrames(f.y, f.u, f.v, align="lsb").lsb == 0                                   # (align is ignored at depth 8)


def test_to_float_and_to_rgb_u8_of_deep_frames():
    from ppmstereo_amd.ppmstereo import YUVFrames
    f = YUVFrames.planar(rand_u16((2, 9, 11), 3, 1024), rand_u16((2, 9, 6), 4, 1024), rand_u16((2, 9, 6), 5, 1024), depth=10, chroma="422")
    levels = f.to_rgb()
    assert levels.dtype == torch.int16 and tuple(levels.shape) == (2, 3, 9, 11)
    assert torch.equal(f.to_float(), levels.float() * (255.0 / 1023)) and f.to_float().dtype == torch.float32
    with pytest.raises(ValueError):
        f.to_rgb_u8()


# ---- YUVFrames on host tensors ---------------------------------------------------------------------------------------------------------
def test_byte_strides_are_read_from_views():
    from ppmstereo_amd.ppmstereo import YUVFrames
    surface = rand_u16((2, 37, 64), 6)                          # a pitched P010 luma surface: 50 of 64 words per row are picture
    uv = rand_u16((2, 19, 32, 2), 7)                            # and its UV plane, 25 of 32 pairs
    f = YUVFrames.p010(surface[:, :, :50], uv[:, :, :25])
    s, fmt = f.view_struct(), f.format_struct()
    assert (f.n, f.height, f.width, len(f), f.depth, f.align, f.chroma) == (2, 37, 50, 2, 10, "msb", "420")
    assert (s.y, s.u, s.v) == (surface.data_ptr(), uv.data_ptr(), uv.data_ptr() + 2)
    assert (s.pitch_y, s.pitch_c, s.step_c, s.frame_stride_y, s.frame_stride_c, s.reserved) == (128, 128, 4, 37 * 128, 19 * 128, 0)
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.sub_x, fmt.sub_y, list(fmt.reserved)) == (2, 10, 6, 1, 1, [0, 0, 0])
    uv2 = rand_u16((2, 37, 32, 2), 8)                           # P210: as many chroma rows as luma rows
    p = YUVFrames.p210(surface[:, :, :50], uv2[:, :, :25])
    s, fmt = p.view_struct(), p.format_struct()
    assert (s.pitch_c, s.step_c, s.frame_stride_c, fmt.sub_x, fmt.sub_y, fmt.lsb) == (128, 4, 37 * 128, 1, 0, 6)
    y8, uv8 = rand_u8((2, 37, 64), 9), rand_u8((2, 37, 32, 2), 10)
    n = YUVFrames.nv16(y8[:, :, :51], uv8[:, :, :26])            # NV16, odd width: ceil
    s, fmt = n.view_struct(), n.format_struct()
    assert (s.pitch_y, s.pitch_c, s.step_c, s.v - s.u, s.frame_stride_c) == (64, 64, 2, 1, 37 * 64)
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.sub_x, fmt.sub_y) == (1, 8, 0, 1, 0)
    u, v = rand_u16((2, 37, 50), 11, 4096), rand_u16((2, 37, 50), 12, 4096)
    q = YUVFrames.planar(surface[:, :, :50], u, v, depth=12, chroma="444")
    s, fmt = q.view_struct(), q.format_struct()
    assert (s.u, s.v, s.pitch_c, s.step_c, s.frame_stride_c) == (u.data_ptr(), v.data_ptr(), 100, 2, 37 * 100)
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.sub_x, fmt.sub_y) == (2, 12, 0, 0, 0)
    one = YUVFrames.planar(surface[:1, :, :50], u[:1], v[:1], depth=12, chroma="444", align="msb")          # a single frame: a plane's size, in bytes
    assert (one.frame_stride_y, one.frame_stride_c, one.lsb) == (2 * (36 * 64 + 50), 2 * 37 * 50, 4)


@pytest.mark.parametrize("depth", [10, 12])
def test_alignment_and_garbage_bits(depth):
    """msb frames x << (16 - depth) with garbage below the sample, and lsb frames with garbage above it, give the levels of clean lsb frames x."""
    from ppmstereo_amd.ppmstereo import YUVFrames
    low = 16 - depth
    planes = [rand_u16(s, 13 + i, 1 << depth) for i, s in enumerate(((2, 9, 11), (2, 5, 6), (2, 5, 6)))]
    clean = YUVFrames.planar(*planes, depth=depth)
    want = clean.to_rgb()
    dirty = lambda t, i: ((t.to(torch.int32) << low) | rand_u16(t.shape, 20 + i, 1 << low).to(torch.int32)).to(torch.uint16)
    msb = YUVFrames.planar(*(dirty(t, i) for i, t in enumerate(planes)), depth=depth, align="msb")
    assert msb.lsb == low and any(bool((p.to(torch.int32) & ((1 << low) - 1)).any()) for p in (msb.y, msb.u, msb.v))
    assert torch.equal(msb.to_rgb(), want)
    above = lambda t, i: (t.to(torch.int32) | (rand_u16(t.shape, 30 + i, 1 << low).to(torch.int32) << depth)).to(torch.uint16)
    lsb = YUVFrames.planar(*(above(t, i) for i, t in enumerate(planes)), depth=depth, align="lsb")
    assert lsb.lsb == 0 and bool((lsb.y.to(torch.int32) >> depth).any()) and torch.equal(lsb.to_rgb(), want)


def test_what_is_no_such_surface_raises():
    from ppmstereo_amd.ppmstereo import YUVFrames
    y, c420, c422, c444 = rand_u16((2, 32, 64), 40), rand_u16((2, 16, 32), 41), rand_u16((2, 32, 32), 42), rand_u16((2, 32, 64), 43)
    for chroma, c in (("420", c420), ("422", c422), ("444", c444)):
        YUVFrames.planar(y, c, c.clone(), depth=10, chroma=chroma)
    wide = rand_u16((2, 32, 128), 44)
    y8, c8 = rand_u8((2, 32, 64), 45), rand_u8((2, 16, 32), 46)
    for bad in (lambda: YUVFrames.planar(y, c420, c420.clone(), depth=10, chroma="422"),           # the chroma shape of another mode
                lambda: YUVFrames.planar(y, c422, c422.clone(), depth=10, chroma="444"),
                lambda: YUVFrames.planar(y, c444, c444.clone(), depth=10, chroma="420"),
                lambda: YUVFrames.planar(y8, c8, c8.clone(), chroma="422"),
                lambda: YUVFrames.planar(wide[:, :, ::2], c420, c420.clone(), depth=10),          # luma with last-dimension stride 2
                lambda: YUVFrames.planar(y, rand_u16((2, 16, 96), 47)[:, :, ::3], rand_u16((2, 16, 96), 48)[:, :, ::3], depth=10),      # chroma step 3
                lambda: YUVFrames.planar(y, c420, rand_u16((2, 16, 64), 49)[:, :, ::2], depth=10),                                      # unequal strides
                lambda: YUVFrames.planar(y8, c8, c8.clone(), depth=10),                           # depth 10 with uint8 planes
                lambda: YUVFrames.planar(y, c420, c420.clone(), depth=8),                         # depth 8 with uint16 planes
                lambda: YUVFrames.planar(y.to(torch.int16), c420.to(torch.int16), c420.to(torch.int16), depth=10),
                lambda: YUVFrames.planar(y, c420, c420.clone(), depth=16), lambda: YUVFrames.planar(y, c420, c420.clone(), depth=10, chroma="411"),
                lambda: YUVFrames.planar(y, c420, c420.clone(), depth=10, align="left"),
                lambda: YUVFrames.planar(y, c420, c420.clone(), depth=10, standard="bt2020"),
                lambda: YUVFrames.p010(y, c420), lambda: YUVFrames.p210(y, c422), lambda: YUVFrames.nv16(y8, rand_u8((2, 16, 32, 2), 50)),
                lambda: YUVFrames.p010(y8, rand_u8((2, 16, 32, 2), 51))):
        with pytest.raises(ValueError):
            bad()
    odd = YUVFrames.planar(rand_u16((1, 37, 51), 52), rand_u16((1, 37, 26), 53), rand_u16((1, 37, 26), 54), depth=12, chroma="422")      # odd sizes: ceil
    assert (odd.height, odd.width, odd.sub_x, odd.sub_y) == (37, 51, 1, 0)


def test_split_slice_and_to_keep_the_format():
    from ppmstereo_amd.ppmstereo import YUVFrames, YUVStereoVideo
    y, uv = rand_u16((3, 32, 128), 55), rand_u16((3, 16, 64, 2), 56)
    p = YUVFrames.p010(y, uv, "bt601", True)
    left, right = p.split_side_by_side()
    l, r = left.view_struct(), right.view_struct()
    assert (r.y - l.y, r.u - l.u, r.v - l.v) == (128, 128, 128) and (l.y, l.u, l.v) == (y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 2)
    assert (r.pitch_y, r.pitch_c, r.step_c, r.frame_stride_y, r.frame_stride_c) == (256, 256, 4, 32 * 256, 16 * 256)
    for half in (left, right):
        assert (half.depth, half.align, half.chroma, half.standard, half.full_range, half.height, half.width) == (10, "msb", "420", "bt601", True, 32, 64)
    full = p.to_rgb()
    assert torch.equal(left.to_rgb(), full[..., :64]) and torch.equal(right.to_rgb(), full[..., 64:])
    top, bottom = p.split_top_bottom()
    assert bottom.view_struct().y - top.view_struct().y == 16 * 256 and bottom.view_struct().u - top.view_struct().u == 8 * 256
    assert torch.equal(bottom.to_rgb(), full[:, :, 16:])
    # 4:4:4 only needs an even packed size; 4:2:2 whole chroma samples across, any even height
    c444 = rand_u16((1, 34, 126), 57, 4096)
    f444 = YUVFrames.planar(rand_u16((1, 34, 126), 58, 4096), c444, c444.clone(), depth=12, chroma="444")
    a, b = f444.split_side_by_side()
    assert (a.width, b.width, b.view_struct().u - a.view_struct().u) == (63, 63, 126) and torch.equal(b.to_rgb(), f444.to_rgb()[..., 63:])
    a, b = f444.split_top_bottom()
    assert (a.height, b.height) == (17, 17) and torch.equal(b.to_rgb(), f444.to_rgb()[:, :, 17:])
    f422 = YUVFrames.nv16(rand_u8((1, 34, 126), 59), rand_u8((1, 34, 63, 2), 60))
    assert f422.split_top_bottom()[1].height == 17
    with pytest.raises(ValueError):
        f422.split_side_by_side()                               # halves of 63 columns: the right one would start between two chroma samples
    with pytest.raises(ValueError):
        YUVFrames.planar(rand_u16((1, 33, 127), 61), c444[:, :33, :127].contiguous(), c444[:, :33, :127].contiguous(), depth=12, chroma="444").split_side_by_side()
    # slicing and to("cpu")
    video = YUVStereoVideo(left, right)
    assert (len(video), video.height, video.width, video.depth) == (3, 32, 64, 10)
    win = video[1:3]
    assert len(win) == 2 and (win.left.depth, win.left.align, win.left.chroma) == (10, "msb", "420")
    assert win.right.view_struct().y == y.data_ptr() + 32 * 256 + 128 and torch.equal(win.right.to_rgb(), right.to_rgb()[1:3])
    assert video.to("cpu").left is left and p.to("cpu") is p     # (nothing to copy: the frames are there)


# ---- RectifyMap on levels ------------------------------------------------------------------------------------------------------------------
def test_apply_levels_and_the_fill_level():
    from ppmstereo_amd.ppmstereo import RectifyMap, StereoRectifier
    from test_ingest_remap import random_map
    for border, fill in (("replicate", 0), ("constant", 0), ("constant", 200), ("constant", 255)):
        m = RectifyMap(*random_map(37, 50, 41, 53, 62), (41, 53), border, fill)
        rgb = rand_u8((2, 3, 41, 53), 63)
        got = m.apply_levels(rgb, 8)
        assert got.dtype == torch.uint8 and torch.equal(got, m.apply_u8(rgb)) and torch.equal(m.apply_levels(rgb), got)
        assert (m.level_fill(), m.level_fill(8), m.view_struct().fill, m.view_struct(8).fill) == (fill,) * 4
        for depth in (10, 12):
            want = (fill << (depth - 8)) | (fill >> (16 - depth))
            assert m.level_fill(depth) == want == m.view_struct(depth).fill and m.view_struct(depth).border == (border == "constant")
    m = RectifyMap.identity(4, 4)
    assert [RectifyMap(m.xy, m.frac, (4, 4), "constant", f).level_fill(d) for f in (0, 255, 128) for d in (10, 12)] == [0, 0, 1023, 4095, 514, 2056]
    # depth 10: every tap of a map that points outside the frame is the fill level; an identity map copies levels
    outside = RectifyMap(torch.full((4, 4, 2), -9, dtype=torch.int16), torch.full((4, 4), 0x155, dtype=torch.int16), (6, 7), "constant", 255)
    levels = rand_u16((2, 3, 6, 7), 64, 1024).to(torch.int16)
    out = outside.apply_levels(levels, 10)
    assert out.dtype == torch.int16 and tuple(out.shape) == (2, 3, 4, 4) and bool((out == 1023).all())
    assert torch.equal(RectifyMap.identity(6, 7).apply_levels(levels, 10), levels)
    both = StereoRectifier(RectifyMap.identity(6, 7), RectifyMap.identity(6, 7)).apply_levels(levels, levels, 10)
    assert torch.equal(both[0], levels) and torch.equal(both[1], levels)
    for bad in (lambda: outside.apply_levels(levels.to(torch.uint8), 10), lambda: outside.apply_levels(levels, 8), lambda: outside.apply_levels(levels, 9)):
        with pytest.raises(ValueError):
            bad()


# ---- the front doors' argument checks ----------------------------------------------------------------------------------------------------
def test_stereo_source_checks_without_a_device():
    from ppmstereo_amd.ppmstereo import RectifyMap, StereoRectifier, YUVFrames, YUVStereoVideo
    from ppmstereo_amd.video import stereo_source
    y, c = rand_u16((2, 32, 64), 65, 1024), rand_u16((2, 16, 32), 66, 1024)
    lsb10 = YUVFrames.planar(y, c, c.clone(), depth=10)
    others = [YUVFrames.planar(y, c, c.clone(), depth=10, align="msb"), YUVFrames.planar(y, c, c.clone(), depth=12),
              YUVFrames.planar(y, rand_u16((2, 32, 32), 67), rand_u16((2, 32, 32), 68), depth=10, chroma="422"),
              YUVFrames.i420(rand_u8((2, 32, 64), 69), rand_u8((2, 16, 32), 70), rand_u8((2, 16, 32), 71))]
    for other in others:
        with pytest.raises(ValueError):
            stereo_source("PPMStereo.forward", lsb10, other)
        with pytest.raises(ValueError):
            YUVStereoVideo(other, lsb10)
    src = stereo_source("PPMStereo.forward", lsb10, YUVFrames.planar(y.clone(), c, c.clone(), depth=10))
    assert (src.n, src.b, src.size, src.depth, src._entry) == (2, 1, (32, 64), 10, "ppms_video_ingest_yuv") and len(src._frames()) == 4
    nv16 = YUVFrames.nv16(rand_u8((2, 32, 64), 72), rand_u8((2, 32, 32, 2), 73))
    assert stereo_source("forward_batch_test", YUVStereoVideo(nv16, nv16))._entry == "ppms_video_ingest_yuv"
    i420 = others[-1]
    plain = stereo_source("forward_batch_test", YUVStereoVideo(i420, i420))                  # 8-bit 4:2:0 keeps its own entry point
    assert plain._entry == "ppms_video_ingest_yuv420" and len(plain._frames()) == 3 and plain.depth == 8
    ident = RectifyMap(RectifyMap.identity(32, 64).xy, RectifyMap.identity(32, 64).frac, (32, 64), "constant", 255)
    rect = stereo_source("forward_batch_test", YUVStereoVideo(lsb10, lsb10), rectify=StereoRectifier(ident, ident))
    assert rect._entry == "ppms_video_ingest_yuv_remap" and [m.fill for m in rect._maps] == [1023, 1023]
    with pytest.raises(ValueError):                                                          # frames of another size than the maps' source
        stereo_source("forward_batch_test", YUVStereoVideo(lsb10, lsb10), rectify=StereoRectifier(RectifyMap.identity(30, 64), RectifyMap.identity(30, 64)))
    left, right = src.float_views()                                                          # the path of other encoder callables: to_float()
    assert torch.equal(left, lsb10.to_float()) and left.dtype == torch.float32 and tuple(right.shape) == (2, 3, 32, 64)
    l2, _ = rect.float_views()
    assert torch.equal(l2, ident.apply_levels(lsb10.to_rgb(), 10).float() * (255.0 / 1023))
