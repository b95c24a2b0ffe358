"""GPU: the packed front doors.  ppms_video_ingest_yuv_packed / ppms_video_ingest_raw_packed (+ _remap) against the UNPACKED doors
ppms_video_ingest_yuv / ppms_video_ingest_raw (+ _remap) on planar frames holding the samples that tests/test_ingest_packed.py's own packer wrote
into the packed rows -- bit-exact, both bf16 planes as int16, into destinations whose every word was non-zero; at x0 = 0 and at an x0 inside a
wider surface, and again with other bits wherever no sample lies.  PPMStereo.forward / forward_batch_test on packed frames against the same calls
on ``unpack()`` (torch.equal).  No tolerance anywhere."""
import pytest
import torch

from ppmstereo_amd.ppmstereo import (OutputSpec, PackedRawFrames, PackedRawStereoVideo, PackedYUVFrames, PackedYUVStereoVideo, RawFrames, RawStereoVideo,
                                     YUVFrames, YUVStereoVideo)
from ingest_util import DEV, bits, fresh, ingest_deep, ingest_packed, ingest_raw, model, rotated_map, same  # noqa: F401  (model: the fixture)
from test_gpu_ingest_remap import smooth_rectifier
from test_ingest_packed import LAYOUTS, PATTERNS, RAW_FORMATS, YUV_FORMATS, packed_raw, packed_yuv

pytestmark = pytest.mark.gpu
RAW_KW = dict(black=70, gains=(1.93, 1.0, 1.52))


# ---- a view in a packed surface on the device, and the planar frames of this file's own making that hold its samples ---------------------------
def yuv_pair(layout, align, N, H, W, x0, P, seed, junk_seed=None, **kw):
    """-> (PackedYUVFrames of columns [x0, x0 + W) of a surface of P columns with 8 bytes of slack a row, the 4:2:2 YUVFrames of the same samples)."""
    depth = LAYOUTS[layout][0]
    data, (Y, U, V) = packed_yuv(layout, align, N, H, P, 8, seed, junk_seed)
    dtype = torch.uint8 if depth == 8 else torch.uint16
    plane = lambda a: torch.from_numpy(a).to(torch.int32).to(dtype).contiguous().to(DEV)
    wc = (W + 1) // 2
    planar = YUVFrames.planar(plane(Y[:, :, x0:x0 + W]), plane(U[:, :, x0 // 2:x0 // 2 + wc]), plane(V[:, :, x0 // 2:x0 // 2 + wc]), depth, "422", "lsb", **kw)
    return PackedYUVFrames(data.to(DEV), W, layout, align, x0=x0, **kw), planar


def raw_pair(packing, depth, pattern, N, H, W, x0, P, seed, junk_seed=None, **kw):
    data, S = packed_raw(packing, depth, N, H, P, 7, seed, junk_seed)
    plane = torch.from_numpy(S[:, :, x0:x0 + W]).to(torch.int32).to(torch.uint16).contiguous().to(DEV)
    return PackedRawFrames(data.to(DEV), W, pattern, depth, packing, x0=x0, **kw), RawFrames(plane, pattern, depth, "lsb", **kw)


def door_equals_door(packed, planar, pad=(7, 13), size=(64, 64), maps=None):
    """packed, planar: (left, right) each.  Both doors write into patterned destinations; -> the packed door's."""
    unpacked = ingest_raw if isinstance(planar[0], RawFrames) else ingest_deep
    n = packed[0].n
    ef, ec = fresh(n, *size)
    unpacked(*planar, *pad, *size, ef.view(), ec.view(), maps)
    f, c = fresh(n, *size)
    ingest_packed(*packed, *pad, *size, f.view(), c.view(), maps)
    torch.cuda.synchronize()
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed
    return f, c


def views(make, x0, P, seed, junk_seed=None, hw=(37, 50)):
    """(the two packed views, the two planar ones): two frames of hw per view; the views' samples differ, `junk_seed` changes nothing but junk."""
    pairs = [make(2, *hw, x0, P, seed + i, None if junk_seed is None else junk_seed + i) for i in range(2)]
    return [p for p, _ in pairs], [q for _, q in pairs]


def plain_and_moved(make, x0, wide):
    """37 x 50 per view -> 64 x 64 at pads (7, 13): the view at column 0 of its own surface, the same with other junk bits (in spare bits, behind the
    last pair or pixel of the last group, in the pitch slack), and at column x0 of a surface `wide` columns wide."""
    packed, planar = views(make, 0, 50, 500)
    f, c = door_equals_door(packed, planar)
    again, planar2 = views(make, 0, 50, 500, junk_seed=900)
    assert all(torch.equal(s, t) for a, b in zip(planar, planar2) for s, t in zip(a._tensors(), b._tensors()))                          # the same samples
    assert not torch.equal(again[0].data, packed[0].data)                                                                              # in other bytes
    f2, c2 = door_equals_door(again, planar2)
    assert torch.equal(bits(f2), bits(f)) and torch.equal(bits(c2), bits(c))
    packed, planar = views(make, x0, wide, 510)
    assert packed[0].view_struct().x0 == x0 and packed[0].data.shape[2] * packed[0].data.element_size() == packed[0].pitch
    door_equals_door(packed, planar)


# ---- the kernel: door equals door ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,align", YUV_FORMATS)
def test_yuv_packed_door_writes_the_unpacked_doors_bits(layout, align):
    """x0 = 26 of 90 columns: inside a v210 group (26 = 4 * 6 + 2), with columns of other samples on both sides of the view."""
    plain_and_moved(lambda N, H, W, x0, P, seed, junk: yuv_pair(layout, align, N, H, W, x0, P, seed, junk, standard="bt601", full_range=layout == "uyvy"), 26, 90)


@pytest.mark.parametrize("packing,depth", RAW_FORMATS)
def test_raw_packed_door_writes_the_unpacked_doors_bits(packing, depth):
    """x0 = 25 of 90 columns: odd, inside a RAW10 group (25 = 6 * 4 + 1) and a RAW12 pair; the pattern stays that of the view's own pixel (0, 0)."""
    plain_and_moved(lambda N, H, W, x0, P, seed, junk: raw_pair(packing, depth, "grbg", N, H, W, x0, P, seed, junk, **RAW_KW), 25, 90)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_mosaic_through_mipi_raw10(pattern):
    make = lambda N, H, W, x0, P, seed, junk: raw_pair("mipi", 10, pattern, N, H, W, x0, P, seed, junk, **RAW_KW)
    door_equals_door(*views(make, 3, 57, 520))
    door_equals_door(*views(make, 0, 2, 522, hw=(2, 2)), pad=(1, 1), size=(4, 4))              # every neighbour is a reflection


def test_tone_table_of_the_frames_own():
    tone = torch.rand(4096, generator=torch.Generator().manual_seed(530)).sort().values * 255.0
    make = lambda N, H, W, x0, P, seed, junk: raw_pair("pfnc", 12, "bggr", N, H, W, x0, P, seed, junk, tone=tone, **RAW_KW)
    packed, planar = views(make, 1, 51, 531)
    assert packed[0].table(DEV).numel() == 4096 and packed[0].table(DEV) is not planar[0].table(DEV) and torch.equal(packed[0].table(DEV), planar[0].table(DEV))
    door_equals_door(packed, planar)


def test_side_by_side_halves_of_one_surface():
    """One YUYV and one RAW12 surface of 100 columns: the right view is the left one's surface at x0 = 50."""
    data, (Y, U, V) = packed_yuv("yuyv", "msb", 2, 37, 100, 8, 540)
    left, right = PackedYUVFrames(data.to(DEV), 100).split_side_by_side()
    assert (left.view_struct().data, left.x0, right.x0) == (right.view_struct().data, 0, 50)
    plane = lambda a: torch.from_numpy(a).to(torch.uint8).contiguous().to(DEV)
    planar = [YUVFrames.planar(plane(Y[:, :, s:s + 50]), plane(U[:, :, s // 2:s // 2 + 25]), plane(V[:, :, s // 2:s // 2 + 25]), 8, "422") for s in (0, 50)]
    door_equals_door([left, right], planar)
    data, S = packed_raw("mipi", 12, 2, 37, 100, 7, 541)
    left, right = PackedRawFrames(data.to(DEV), 100, "rggb", 12, "mipi", **RAW_KW).split_side_by_side()
    planar = [RawFrames(torch.from_numpy(S[:, :, s:s + 50]).to(torch.int32).to(torch.uint16).contiguous().to(DEV), "rggb", 12, "lsb", **RAW_KW) for s in (0, 50)]
    door_equals_door([left, right], planar)


# ---- the _remap twins -----------------------------------------------------------------------------------------------------------------------
def remapped(make, x0, wide):
    """Source frames 40 x 56 -> rectified 37 x 50 -> 64 x 64; the views turn in opposite directions, the maps' corners lie outside the source frame,
    in both border modes; against the unpacked door's _remap twin."""
    packed, planar = views(make, x0, wide, 550, hw=(40, 56))
    for border, fill in (("replicate", 0), ("constant", 255)):
        maps = rotated_map(37, 50, 40, 56, 0.21, 1.2, border, fill), rotated_map(37, 50, 40, 56, -0.17, 1.25, border, fill)
        door_equals_door(packed, planar, maps=maps)


@pytest.mark.parametrize("layout,align", YUV_FORMATS)
def test_yuv_packed_remap_writes_the_unpacked_remaps_bits(layout, align):
    remapped(lambda N, H, W, x0, P, seed, junk: yuv_pair(layout, align, N, H, W, x0, P, seed, junk), 2, 60)


@pytest.mark.parametrize("packing,depth", RAW_FORMATS)
def test_raw_packed_remap_writes_the_unpacked_remaps_bits(packing, depth):
    remapped(lambda N, H, W, x0, P, seed, junk: raw_pair(packing, depth, "gbrg", N, H, W, x0, P, seed, junk, **RAW_KW), 3, 61)


# ---- the model: forward on packed frames is forward on unpack() ------------------------------------------------------------------------------
def test_model_forward_on_a_yuyv_side_by_side_frame(model):
    """One (3, 64, 512) YUYV surface of a stereo head, split: two views of 64 x 256 over one buffer."""
    data, _ = packed_yuv("yuyv", "msb", 3, 64, 512, 0, 560)
    left, right = PackedYUVFrames(data.to(DEV), 512).split_side_by_side()
    assert left.data.data_ptr() == right.data.data_ptr() and (right.x0, right.width) == (256, 256)
    d, u = model.forward(left, right, iters=4, test_mode=True)
    rd, ru = model.forward(left.unpack(), right.unpack(), iters=4, test_mode=True)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.isfinite(d).all() and torch.equal(d, rd) and torch.equal(u, ru)
    with pytest.raises(ValueError):                              # the two views must be one kind of frame
        model.forward(left, PackedYUVFrames(right.data, 256, "uyvy", x0=256), iters=4, test_mode=True)
    with pytest.raises(TypeError):
        model.forward(left, right.unpack(), iters=4, test_mode=True)


def test_model_v210_video_from_the_host(model):
    """(3, 60, 250) v210 frames on the host -> 64 x 256, one window: the packed bytes are what crosses to the device."""
    views_ = [PackedYUVFrames(packed_yuv("v210", "msb", 3, 60, 250, 0, 561 + i)[0], 250, "v210") for i in range(2)]
    video = PackedYUVStereoVideo(*views_)
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    out = run(video)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and torch.isfinite(out["disparity"]).all()
    assert same(out, run(YUVStereoVideo(*(v.unpack() for v in views_))))
    on_device = video.to(DEV)
    assert on_device.left.data.is_cuda and on_device.left.data.dtype == torch.uint8 and on_device.left.data.shape[2] == 16 * 42
    assert same(run(on_device), out)


def test_model_mipi_raw10_with_rectify(model):
    """Raw 70 x 262 RAW10 frames of an unrectified rig -> rectified 60 x 250."""
    r = smooth_rectifier(60, 250, 70, 262, 7, "constant", 200)
    views_ = [PackedRawFrames(packed_raw("mipi", 10, 3, 70, 262, 3, 563 + i)[0], 262, "grbg", 10, "mipi", black=64, gains=(1.5, 1.0, 1.8)) for i in range(2)]
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, rectify=r)
    out = run(PackedRawStereoVideo(*views_))
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and same(out, run(RawStereoVideo(*(v.unpack() for v in views_))))


def test_model_quantised_output_of_a_packed_raw_video(model):
    views_ = [PackedRawFrames(packed_raw("pfnc", 12, 3, 60, 250, 0, 565 + i)[0], 250, "bggr", 12, "pfnc", black=256) for i in range(2)]
    spec = OutputSpec("u16", uncertainty="u8")
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, output=spec)
    q, qref = run(PackedRawStereoVideo(*views_)), run(RawStereoVideo(*(v.unpack() for v in views_)))
    assert q["disparity"].dtype == torch.uint16 and q["uncertainties"].dtype == torch.uint8 and tuple(q["disparity"].shape) == (3, 1, 60, 250)
    for k in ("disparity", "uncertainties"):
        assert torch.equal(q[k].view(torch.uint8), qref[k].view(torch.uint8))
