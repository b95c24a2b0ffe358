"""CPU: the decoded-video front door.  ppms_video_ingest_yuv420 (NV12 / I420 frames -> the first-layer operands of both encoders)
refuses bad arguments before touching a device (its ABI: tests/test_ingest_doors.py);
yuv_matrix / YUVFrames.to_rgb_u8 are the conversion the header states (against float64), and YUVFrames / YUVStereoVideo read pointers and
strides from views without copying.  No device compute."""
import ctypes
import functools
import itertools

import pytest
import torch

from ingest_util import EINVAL, call, lib, rand_u8, remap_view, yuv_view  # noqa: F401  (lib: the fixture)

NAME = "ppms_video_ingest_yuv420"


# ---- argument refusal: NV12 frames of 37 x 50 (chroma 19 x 25) in surfaces of pitch 64, two frames, padded to 64 x 64 ----------------
_view = functools.partial(yuv_view, y=0x100000, u=0x200000, v=0x200001, fsy=37 * 64, fsc=19 * 64, pitch_y=64, pitch_c=64, step_c=2)


def _call(lib, left=None, right=None, null=(), twin=False, **kw):
    """kw: fields of the matrix, and the call's geometry (ingest_util.call).  twin: through the _remap twin, with maps whose source frame is H0 x W0."""
    from ppmstereo_amd.ppmstereo import yuv_matrix
    mat = yuv_matrix()
    for k in [k for k in kw if hasattr(mat, k)]:
        setattr(mat, k, kw.pop(k))
    maps = [remap_view(hs=kw.get("H0", 37), ws=kw.get("W0", 50))] * 2 if twin else ()
    return call(lib, NAME + "_remap" * twin, [_view(**(left or {})), _view(**(right or {})), mat], maps, null=null, **kw)


# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(lut=0)),          # NULL view / matrix / table
       ("null plane", dict(left=dict(y=0))), ("null plane", dict(right=dict(u=0))), ("null plane", dict(left=dict(v=0))),
       ("step_c", dict(left=dict(step_c=0))), ("step_c", dict(right=dict(step_c=3))),
       ("pitch_y", dict(left=dict(pitch_y=49))), ("pitch_y", dict(right=dict(pitch_y=49))),                             # pitch_y < W0 = 50
       ("pitch_c", dict(left=dict(pitch_c=48))), ("pitch_c", dict(right=dict(pitch_c=24, step_c=1))),                   # < 2 * 24 + 1, < 25
       ("frame_stride_y", dict(left=dict(fsy=36 * 64 + 49))), ("frame_stride_c", dict(right=dict(fsc=18 * 64 + 48))),   # frames overlap
       ("shift", dict(shift=7)), ("shift", dict(shift=21)),
       ("reserved", dict(left=dict(reserved=1))), ("reserved", dict(right=dict(reserved=-1))), ("reserved", dict(reserved=1)),
       ("skipped", dict(fnet=False, cnet=False)),
       ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
       ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
       ("positive", dict(N=0)), ("positive", dict(H0=0)),
       ("coefficient", dict(cy=-1)), ("coefficient", dict(crv=4 << 14)), ("coefficient", dict(y_off=256))]


@pytest.mark.parametrize("about,bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for _, b in BAD])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert _call(lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_yuv420" in msg and about.encode() in msg, (bad, msg)


def test_destination_views_follow_img_s2d_contract(lib):
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import yuv_matrix
    v, m = _view(fsy=32 * 64, fsc=16 * 64), yuv_matrix()
    call = lambda f, c: lib.ppms_video_ingest_yuv420(ctypes.byref(v), ctypes.byref(v), ctypes.byref(m), 1, 32, 32, 0, 0, 32, 32, 0x3000, f, c, None)
    ok = L.SP(0x10000, 0x20000, 32, 32)
    for view in (L.SP(0x10000, None, 32, 32), L.SP(0x10000, 0x20000, 32, 8), L.SP(0x10000, 0x20000, 36, 32), L.SP(0x10008, 0x20000, 32, 32)):
        assert call(view, L.SP(None, None, 0, 0)) == EINVAL
        assert b"destination" in lib.ppms_last_error() and b"video_ingest_yuv420" in lib.ppms_last_error()
    assert call(ok, L.SP(0x10000, 0x20000, 40, 40)) == EINVAL      # the k = 4 operand holds 48 values


# ---- the conversion ------------------------------------------------------------------------------------------------------------------
STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
COMBOS = list(itertools.product(("bt709", "bt601"), (False, True)))


def float64_rgb(y, u, v, standard, full_range):
    """The YCbCr -> RGB equations in float64, rounded half up and clamped (y, u, v: int64 tensors of one shape) -> (3, ...) int64."""
    kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    sy, sc, off = (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)
    d, e, f = (y - off).double() * sy, (u - 128).double() * sc, (v - 128).double() * sc
    r = d + 2.0 * (1.0 - kr) * f
    g = d - 2.0 * kb * (1.0 - kb) / kg * e - 2.0 * kr * (1.0 - kr) / kg * f
    b = d + 2.0 * (1.0 - kb) * e
    return torch.floor(torch.stack([r, g, b]) + 0.5).clamp(0, 255).long()


def one_pixel_frames(y, u, v, standard, full_range):
    """Every (Y, U, V) triple as a frame of one pixel."""
    from ppmstereo_amd.ppmstereo import YUVFrames
    as_plane = lambda t: t.to(torch.uint8).reshape(-1, 1, 1)
    return YUVFrames(as_plane(y), as_plane(u), as_plane(v), standard, full_range)


@pytest.mark.parametrize("standard,full_range", COMBOS)
def test_yuv_matrix_against_float64(standard, full_range):
    """A 32-step grid of (Y, U, V) plus the corners: at shift = 14 the rounded coefficients move a sum by less than 0.03 of a level
    (at most 3 coefficients in a sum, each off by <= 2^-15, times an operand <= 255), so the integer result may differ from the float64 one
    near ties only."""
    from ppmstereo_amd.ppmstereo import yuv_matrix
    levels = torch.tensor(sorted(set(range(0, 256, 32)) | {255}))
    y, u, v = (t.reshape(-1) for t in torch.meshgrid(levels, levels, levels, indexing="ij"))
    assert {(0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 0, 255)} <= set(zip(y.tolist(), u.tolist(), v.tolist()))
    got = one_pixel_frames(y, u, v, standard, full_range).to_rgb_u8()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (y.numel(), 3, 1, 1)
    want = float64_rgb(y, u, v, standard, full_range)                        # (3, n)
    diff = (got.reshape(-1, 3).long().T - want).abs()
    assert int(diff.max()) <= 1, int(diff.max())
    m = yuv_matrix(standard, full_range)
    assert (m.shift, m.reserved, m.y_off) == (14, 0, 0 if full_range else 16)
    kr, kb = STANDARDS[standard]
    sc = 1.0 if full_range else 255.0 / 224.0
    assert m.crv == round(sc * 2 * (1 - kr) * 16384) and m.cbu == round(sc * 2 * (1 - kb) * 16384)
    assert m.cy == (16384 if full_range else round(255.0 / 219.0 * 16384))
    assert m.cgu == round(sc * 2 * kb * (1 - kb) / (1 - kr - kb) * 16384) and m.cgv == round(sc * 2 * kr * (1 - kr) / (1 - kr - kb) * 16384)


@pytest.mark.parametrize("standard", ["bt709", "bt601"])
def test_grey_axis(standard):
    grey = torch.full((256,), 128)
    full = one_pixel_frames(torch.arange(256), grey, grey, standard, True).to_rgb_u8().reshape(256, 3)
    assert torch.equal(full, torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3))
    lim = one_pixel_frames(torch.tensor([16, 235, 0, 255]), grey[:4], grey[:4], standard, False).to_rgb_u8().reshape(4, 3)
    assert lim.tolist() == [[0, 0, 0], [255, 255, 255], [0, 0, 0], [255, 255, 255]]


def test_yuv_matrix_refuses_what_the_kernel_refuses():
    from ppmstereo_amd.ppmstereo import yuv_matrix
    for kw in (dict(standard="bt2020"), dict(shift=7), dict(shift=21)):
        with pytest.raises(ValueError):
            yuv_matrix(**kw)
    assert yuv_matrix(shift=20).cy == round(255.0 / 219.0 * (1 << 20))


# ---- YUVFrames / YUVStereoVideo on host tensors ----------------------------------------------------------------------------------------
def test_strides_are_read_from_views():
    from ppmstereo_amd.ppmstereo import YUVFrames
    surface = rand_u8((2, 37, 64), 1)                           # a pitched luma surface: 50 of 64 bytes per row are picture
    uv = rand_u8((2, 19, 32, 2), 2)                             # and its UV plane, 25 of 32 pairs
    f = YUVFrames.nv12(surface[:, :, :50], uv[:, :, :25])
    s = f.view_struct()
    assert (f.n, f.height, f.width, len(f)) == (2, 37, 50, 2)
    assert (s.y, s.u, s.v) == (surface.data_ptr(), uv.data_ptr(), uv.data_ptr() + 1)
    assert (s.pitch_y, s.pitch_c, s.step_c, s.frame_stride_y, s.frame_stride_c, s.reserved) == (64, 64, 2, 37 * 64, 19 * 64, 0)
    u, v = rand_u8((2, 19, 25), 3), rand_u8((2, 19, 25), 4)
    p = YUVFrames.i420(surface[:, :, :50], u, v).view_struct()
    assert (p.u, p.v, p.pitch_c, p.step_c, p.frame_stride_c) == (u.data_ptr(), v.data_ptr(), 25, 1, 19 * 25)
    one = YUVFrames(surface[:1, :, :50], u[:1], v[:1]).view_struct()                # a single frame: the frame strides are a plane's size
    assert (one.frame_stride_y, one.frame_stride_c) == (36 * 64 + 50, 19 * 25)


def test_what_is_no_420_surface_raises():
    from ppmstereo_amd.ppmstereo import YUVFrames
    y, u, v = rand_u8((2, 32, 64), 5), rand_u8((2, 16, 32), 6), rand_u8((2, 16, 32), 7)
    YUVFrames(y, u, v)
    wide = rand_u8((2, 32, 128), 8)
    for bad in (lambda: YUVFrames(wide[:, :, ::2], u, v),                       # luma with last-dimension stride 2
                lambda: YUVFrames(y, u, rand_u8((2, 16, 64), 9)[:, :, ::2]),    # u and v with different strides
                lambda: YUVFrames(y, rand_u8((2, 16, 96), 10)[:, :, ::3], rand_u8((2, 16, 96), 11)[:, :, ::3]),       # chroma step 3
                lambda: YUVFrames(y, u[:, :15], v[:, :15]), lambda: YUVFrames(y, u, v[:1]),                           # wrong chroma size
                lambda: YUVFrames(y.float(), u, v), lambda: YUVFrames(y[0], u[0], v[0]),
                lambda: YUVFrames(y, u, v, standard="bt2020"),
                lambda: YUVFrames.nv12(y, u)):
        with pytest.raises(ValueError):
            bad()
    odd = YUVFrames(rand_u8((1, 37, 51), 12), rand_u8((1, 19, 26), 13), rand_u8((1, 19, 26), 14))     # odd sizes are legal: ceil
    assert (odd.height, odd.width) == (37, 51)


def test_packed_frames_split_without_a_copy():
    from ppmstereo_amd.ppmstereo import YUVFrames
    y, uv = rand_u8((2, 32, 128), 15), rand_u8((2, 16, 64, 2), 16)
    nv = YUVFrames.nv12(y, uv)
    l, r = (f.view_struct() for f in nv.split_side_by_side())
    assert (r.y - l.y, r.u - l.u, r.v - l.v) == (64, 64, 64) and (l.y, l.u, l.v) == (y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 1)
    assert (r.pitch_y, r.pitch_c, r.step_c, r.frame_stride_y, r.frame_stride_c) == (128, 128, 2, 32 * 128, 16 * 128)
    u, v = rand_u8((2, 16, 64), 17), rand_u8((2, 16, 64), 18)
    left, right = YUVFrames.i420(y, u, v).split_side_by_side()
    l, r = left.view_struct(), right.view_struct()
    assert (r.y - l.y, r.u - l.u, r.v - l.v) == (64, 32, 32) and (r.pitch_c, r.step_c) == (64, 1)
    assert (left.height, left.width, right.height, right.width) == (32, 64, 32, 64)
    full = YUVFrames.i420(y, u, v).to_rgb_u8()
    assert torch.equal(left.to_rgb_u8(), full[..., :64]) and torch.equal(right.to_rgb_u8(), full[..., 64:])
    top, bottom = nv.split_top_bottom()
    t, b = top.view_struct(), bottom.view_struct()
    assert (b.y - t.y, b.u - t.u) == (16 * 128, 8 * 128) and (top.height, top.width) == (16, 128)
    assert torch.equal(bottom.to_rgb_u8(), nv.to_rgb_u8()[:, :, 16:])
    for shape, split in (((1, 32, 127), "split_side_by_side"), ((1, 33, 128), "split_top_bottom"),
                         ((1, 32, 126), "split_side_by_side"), ((1, 34, 128), "split_top_bottom")):     # odd; and even with odd halves
        n, h, w = shape
        f = YUVFrames(rand_u8(shape, 19), rand_u8((n, (h + 1) // 2, (w + 1) // 2), 20), rand_u8((n, (h + 1) // 2, (w + 1) // 2), 21))
        with pytest.raises(ValueError):
            getattr(f, split)()


def test_stereo_video_len_slice_and_checks():
    from ppmstereo_amd.ppmstereo import YUVFrames, YUVStereoVideo
    y, uv = rand_u8((7, 32, 128), 22), rand_u8((7, 16, 64, 2), 23)
    left, right = YUVFrames.nv12(y, uv).split_side_by_side()
    video = YUVStereoVideo(left, right)
    assert (len(video), video.height, video.width) == (7, 32, 64)
    win = video[2:5]
    assert isinstance(win, YUVStereoVideo) and len(win) == 3
    assert win.left.view_struct().y == y.data_ptr() + 2 * 32 * 128 and win.right.view_struct().u == uv.data_ptr() + 2 * 16 * 128 + 64
    assert torch.equal(win.right.to_rgb_u8(), right.to_rgb_u8()[2:5])
    assert len(video[5:20]) == 2 and video.to("cpu").left is left             # (nothing to copy: the frames are there)
    with pytest.raises(ValueError):
        YUVStereoVideo(left, right[:3])
    with pytest.raises(ValueError):
        YUVStereoVideo(left, YUVFrames(right.y, right.u, right.v, standard="bt601"))
    with pytest.raises(TypeError):
        YUVStereoVideo(left, y)
