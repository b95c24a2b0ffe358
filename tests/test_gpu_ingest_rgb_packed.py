"""GPU: the interleaved-RGB front door.  ppms_video_ingest_rgb_packed (+ _remap) on surfaces that tests/test_ingest_rgb_packed.py's own packer wrote:
the 8-bit layouts against ppms_video_ingest_u8 (+ _remap) on the planar bytes, the word and 10-bit layouts against the float path's own op chain fed
``levels * (255 / (2^depth - 1))`` of the levels the packer was given (and this file's restatement of the remap on them) -- bit-exact, both bf16 planes
as int16, into destinations whose every word was non-zero; at x0 = 0 and at an x0 inside a wider surface, and again with other bits wherever no
level lies.  The colour twins against ``colour_bytes``; PPMStereo.forward / forward_batch_test on interleaved frames against the same calls on the
planar uint8 or float video (torch.equal).  No tolerance anywhere."""
import pytest
import torch

from colour_util import ColourDest, padded_float
from ingest_util import (DEV, bits, float_path_operands, fresh, ingest, ingest_door, model, rand_u8, restated_remap, rotated_map, same)  # noqa: F401  (model: the fixture)
from ppmstereo_amd.ppmstereo import OutputSpec, PackedRGBFrames, PackedRGBStereoVideo, RectifyMap, StereoRectifier, colour_bytes, level_lut, stereo_source
from test_gpu_block import W
from test_gpu_ingest_remap import smooth_rectifier
from test_ingest_rgb_packed import BYTE_LAYOUTS, DEEP_FORMATS, LAYOUTS, packed_rgb

pytestmark = pytest.mark.gpu
PAD = [7, 7, 13, 14]                                                  # F.pad's list for 37 x 50 -> 64 x 64 at pads (7, 13)


# ---- a view in an interleaved surface on the device, and the levels of this file's own making that it holds -------------------------------------
def view(layout, depth, align, N, H, Wd, x0, P, seed, junk_seed=None, levels=None):
    """-> (PackedRGBFrames of columns [x0, x0 + Wd) of a surface of P columns with 8 bytes of slack a row, their levels (N, 3, H, Wd) int64 on the
    device).  unpack() must give those levels: the package's definition is the packer's."""
    data, S = packed_rgb(layout, depth, align, N, H, P, 8, seed, junk_seed, levels)
    frames, own = PackedRGBFrames(data.to(DEV), Wd, layout, depth, align, x0=x0), S[:, :, :, x0:x0 + Wd].contiguous().to(DEV)
    assert frames.data.is_cuda and torch.equal(frames.unpack().long(), own)
    return frames, own


def views(layout, depth, align, x0, P, seed, junk_seed=None, hw=(37, 50), N=2):
    """(the two views, their levels): N frames of hw per view; the views' levels differ, `junk_seed` changes nothing but junk."""
    pairs = [view(layout, depth, align, N, *hw, x0, P, seed + i, None if junk_seed is None else junk_seed + i) for i in range(2)]
    return [p for p, _ in pairs], [s for _, s in pairs]


def ingest_rgb(left, right, pad_left, pad_top, H, Wd, fview, cview, maps=None):
    """The interleaved door on two PackedRGBFrames of one format, with the level table of their depth."""
    assert left.format_fault(right) is None
    lut = level_lut(DEV, left.depth)
    assert lut.numel() == 1 << left.depth
    head = left.view_struct(), right.view_struct(), left.format_struct()
    return ingest_door("rgb_packed", head, maps, left.n, (left.height, left.width), pad_left, pad_top, H, Wd, lut, fview, cview)


# ---- the expectations ---------------------------------------------------------------------------------------------------------------------------
def as_float(levels, depth):
    """What the reference would be given: the float video of the levels."""
    return levels.float() * (255.0 / (2 ** depth - 1))


def remapped_levels(levels, m: RectifyMap, depth):
    """levels (N, 3, Hs, Ws) int64 -> (N, 3, H0, W0) int64 by ingest_util's restated remap; a tap outside the frame is, in constant mode, the byte
    `fill` with its top bits repeated below it."""
    return restated_remap(levels, m.xy, m.frac, m.border, m.fill * 2 ** (depth - 8) + m.fill // 2 ** (16 - depth), 2 ** depth - 1)


def expected(levels, depth, pad, size, maps=None):
    """Both destinations as they must be.  Depth 8: ppms_video_ingest_u8 (+ _remap) on the planar bytes; deeper: the float path's two operands for
    the float video of the levels (behind the restated remap, if there are maps)."""
    ll, rl = levels
    n, _, hs, ws = ll.shape
    if depth == 8:
        lu, ru = ll.to(torch.uint8).contiguous(), rl.to(torch.uint8).contiguous()
        ef, ec = fresh(n, *size)
        ingest(lu.data_ptr(), ru.data_ptr(), 3 * hs * ws, n, hs, ws, pad[0], pad[2], *size, ef.view(), ec.view(), maps)
        torch.cuda.synchronize()
        return ef, ec
    if maps is not None:
        ll, rl = remapped_levels(ll, maps[0], depth), remapped_levels(rl, maps[1], depth)
    ef, ec, H, Wd = float_path_operands(as_float(ll, depth), as_float(rl, depth), pad)
    torch.cuda.synchronize()
    assert (H, Wd) == tuple(size)
    return ef, ec


def door_writes(frames, levels, pad=PAD, size=(64, 64), maps=None):
    """frames, levels: (left, right) each.  The door writes into patterned destinations what `expected` says; -> its destinations."""
    ef, ec = expected(levels, frames[0].depth, pad, size, maps)
    f, c = fresh(frames[0].n, *size)
    ingest_rgb(*frames, pad[0], pad[2], *size, f.view(), c.view(), maps)
    torch.cuda.synchronize()
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed
    return f, c


def plain_and_moved(layout, depth, align, seed):
    """37 x 50 per view -> 64 x 64 at pads (7, 13): the view at column 0 of its own surface, the same with other junk (alpha, spare bits of words,
    bits 30 and 31, the pitch slack), and at column 25 of a surface 90 columns wide with other pixels on both sides."""
    frames, levels = views(layout, depth, align, 0, 50, seed)
    f, c = door_writes(frames, levels)
    again, levels2 = views(layout, depth, align, 0, 50, seed, junk_seed=900)
    stored = lambda v: v.data.view(torch.int16) if v.data.dtype == torch.uint16 else v.data             # (the same bits, in a type the device compares)
    assert all(torch.equal(a, b) for a, b in zip(levels, levels2)) and not torch.equal(stored(again[0]), stored(frames[0]))      # the same levels in other bytes
    f2, c2 = door_writes(again, levels2)
    assert torch.equal(bits(f2), bits(f)) and torch.equal(bits(c2), bits(c))
    frames, levels = views(layout, depth, align, 25, 90, seed + 10)
    s = frames[0].view_struct()
    assert s.x0 == 25 and s.pitch == frames[0].data.shape[2] * frames[0].data.element_size() == (1, 2, 4)[LAYOUTS[layout][0]] * LAYOUTS[layout][1] * 90 + 8
    door_writes(frames, levels)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", BYTE_LAYOUTS)
def test_byte_layouts_write_the_uint8_doors_bits(layout):
    plain_and_moved(layout, 8, "msb", 500)


@pytest.mark.parametrize("layout,depth,align", DEEP_FORMATS, ids=[f"{l}-{d}-{a}" for l, d, a in DEEP_FORMATS])
def test_word_and_ten_bit_layouts_write_the_float_paths_bits(layout, depth, align):
    """Dirty low bits (msb), high bits (lsb) and bits 30, 31 come with the packer's junk; the second run changes them and nothing else."""
    plain_and_moved(layout, depth, align, 520)


@pytest.mark.parametrize("layout,depth,align", [("x2rgb10", 10, "msb"), ("rgba64", 10, "lsb"), ("bgr48", 12, "msb"), ("rgb48", 12, "lsb")])
def test_every_level_in_every_channel(layout, depth, align):
    """One 64 x 64 frame per view whose three channels each hold every level of `depth` bits, each in its own order: both ends of the table are used."""
    g = torch.Generator().manual_seed(530 + depth)
    frames, levels = [], []
    for i in range(2):
        S = torch.stack([torch.randperm(4096, generator=g) % (1 << depth) for _ in range(3)]).reshape(1, 3, 64, 64)
        assert all(sorted(S[0, ch].reshape(-1).tolist()) == sorted(list(range(1 << depth)) * (4096 >> depth)) for ch in range(3))
        f, own = view(layout, depth, align, 1, 64, 64, 0, 64, 531 + i, levels=S.numpy())
        frames.append(f), levels.append(own)
    door_writes(frames, levels, [0, 0, 0, 0])


@pytest.mark.parametrize("layout,depth,align", [("bgr24", 8, "msb"), ("argb", 8, "msb"), ("rgb48", 12, "msb"), ("x2bgr10", 10, "msb")])
def test_one_pixel_frame_fills_the_padded_image(layout, depth, align):
    """A 1 x 1 frame into 4 x 4 at pads (1, 1): every output pixel, every phase of both operands, is that pixel."""
    frames, levels = views(layout, depth, align, 0, 1, 540, hw=(1, 1), N=1)
    f, c = door_writes(frames, levels, [1, 2, 1, 2], (4, 4))
    fb, cb = bits(f)[:, :, :12].reshape(2, 2, 4, 4, 3), bits(c)[:, :, :48].reshape(2, 1, 16, 3)      # (plane, image, pixel, phase, channel)
    assert bool((fb == fb[:, :, :1, :1]).all()) and bool((cb == cb[:, :, :1]).all()) and not torch.equal(fb[:, 0], fb[:, 1])


@pytest.mark.parametrize("layout,depth", [("bgra", 8), ("x2rgb10", 10)])
def test_skipped_destinations_stay_untouched(layout, depth):
    """32 x 64, T = 3, no padding; a destination with hi == NULL is skipped and stays as it was."""
    frames, levels = views(layout, depth, "msb", 0, 64, 550, hw=(32, 64), N=3)
    ef, ec = expected(levels, depth, [0, 0, 0, 0], (32, 64))
    for skip in ("cnet", "fnet"):
        f, c = fresh(3, 32, 64)
        before_f, before_c = bits(f).clone(), bits(c).clone()
        fv, cv = f.view(), c.view()
        if skip == "cnet":
            cv.hi = None                                         # (lo, ld, c stay set: hi == NULL alone must be enough to skip)
        else:
            fv.hi = None
        ingest_rgb(*frames, 0, 0, 32, 64, fv, cv)
        torch.cuda.synchronize()
        if skip == "cnet":
            assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), before_c)
        else:
            assert torch.equal(bits(c), bits(ec)) and torch.equal(bits(f), before_f)


def test_frame_strides_past_2_to_31_bytes():
    """Frame 1 of each view lies more than 2^31 bytes behind frame 0: the source offsets are 64-bit arithmetic.  One buffer of 16-bit words, shared
    by the two views' (different) pictures at different offsets: rgb48 of 12 bits, 8 x 12 pixels."""
    H0, W0, stride = 8, 12, (1 << 30) + 2049                                                  # in 16-bit elements
    row = 3 * W0
    buf = torch.empty(stride + 2 * H0 * row, dtype=torch.uint16, device=DEV)
    frames, levels = [], []
    for i in range(2):
        src, own = view("rgb48", 12, "msb", 2, H0, W0, 0, W0, 560 + i)
        surface = torch.as_strided(buf, (2, H0, row), (stride, row, 1), i * H0 * row)
        surface.copy_(src.data[:, :, :row])
        frames.append(PackedRGBFrames(surface, W0, "rgb48", 12))
        assert frames[-1].view_struct().frame_stride == 2 * stride > 1 << 31
        levels.append(own)                                      # (the levels of `src`, whose rows the surface holds)
    door_writes(frames, levels, [0, 0, 0, 0], (8, 12))
    del buf, frames


# ---- the _remap twins ---------------------------------------------------------------------------------------------------------------------------
REMAP_FORMATS = [(l, 8, "msb") for l in ("bgr24", "rgba", "xbgr")] + [("rgb48", 10, "msb"), ("bgra64", 12, "lsb"), ("x2rgb10", 10, "msb"), ("x2bgr10", 10, "msb")]


@pytest.mark.parametrize("layout,depth,align", REMAP_FORMATS, ids=[f"{l}-{d}-{a}" for l, d, a in REMAP_FORMATS])
def test_remap_twin_on_rotated_maps_in_both_border_modes(layout, depth, align):
    """Source frames 40 x 56 at column 3 of a surface of 61 -> rectified 37 x 50 -> 64 x 64; the views turn in opposite directions, the maps' corners
    lie outside the source frame; `fill` is the top level.  8 bits: the u8 _remap door's bits on the planar bytes; deeper: the restated remap."""
    frames, levels = views(layout, depth, align, 3, 61, 570, hw=(40, 56))
    for border, fill in (("replicate", 0), ("constant", 255)):
        maps = rotated_map(37, 50, 40, 56, 0.21, 1.2, border, fill), rotated_map(37, 50, 40, 56, -0.17, 1.25, border, fill)
        assert maps[0].view_struct(depth).fill == (2 ** depth - 1 if fill else 0)
        door_writes(frames, levels, maps=maps)


@pytest.mark.parametrize("layout,depth,align", [("bgr24", 8, "msb"), ("rgb48", 12, "msb"), ("x2rgb10", 10, "msb")])
def test_remap_identity_maps_give_the_plain_doors_bits(layout, depth, align):
    ident = RectifyMap.identity(37, 50, device=DEV)
    frames, levels = views(layout, depth, align, 25, 90, 580)
    f, c = door_writes(frames, levels)
    rf, rc = door_writes(frames, levels, maps=(ident, ident))
    assert torch.equal(bits(rf), bits(f)) and torch.equal(bits(rc), bits(c))


# ---- halves and crops of (N, H, W, C) tensors ---------------------------------------------------------------------------------------------------
def planar_levels(hwc, pick):
    """(N, H, W, C) uint8 on the device -> the planar int64 levels (N, 3, H, W) of its channels `pick` = (R, G, B)."""
    return hwc.permute(0, 3, 1, 2)[:, list(pick)].contiguous().long()


def test_side_by_side_and_top_bottom_halves_of_one_tensor():
    wide = rand_u8((2, 37, 100, 3), 590).to(DEV)
    left, right = PackedRGBFrames.from_hwc(wide).split_side_by_side()
    assert (left.view_struct().data, left.x0, right.x0, right.pitch) == (right.view_struct().data, 0, 50, 300)
    door_writes([left, right], [planar_levels(wide[:, :, :50], (2, 1, 0)), planar_levels(wide[:, :, 50:], (2, 1, 0))])
    tall = rand_u8((2, 74, 50, 4), 591).to(DEV)
    top, bottom = PackedRGBFrames.from_hwc(tall, "argb").split_top_bottom()
    assert bottom.view_struct().data - top.view_struct().data == 37 * 200 and (top.frame_stride, top.height) == (74 * 200, 37)
    door_writes([top, bottom], [planar_levels(tall[:, :37], (1, 2, 3)), planar_levels(tall[:, 37:], (1, 2, 3))])


def test_strided_crops_of_a_larger_tensor():
    big = rand_u8((2, 45, 70, 4), 592).to(DEV)
    a, b = big[:, 3:40, 5:55], big[:, 8:45, 20:70]
    left, right = PackedRGBFrames.from_hwc(a, "bgra"), PackedRGBFrames.from_hwc(b, "bgra")
    assert (left.data.data_ptr(), left.pitch, left.frame_stride, left.x0) == (a.data_ptr(), 280, 45 * 280, 0) and right.data.data_ptr() == b.data_ptr()
    door_writes([left, right], [planar_levels(a, (2, 1, 0)), planar_levels(b, (2, 1, 0))])


# ---- the colour twins ---------------------------------------------------------------------------------------------------------------------------
COLOUR_FORMATS = [("bgr24", 8, "msb"), ("argb", 8, "msb"), ("rgb48", 12, "msb"), ("x2bgr10", 10, "msb")]


@pytest.mark.parametrize("twin", [False, True], ids=["plain", "remap"])
@pytest.mark.parametrize("layout,depth,align", COLOUR_FORMATS, ids=[f"{l}-{d}" for l, d, _ in COLOUR_FORMATS])
def test_colour_twins_write_colour_bytes_of_the_float_video(layout, depth, align, twin):
    """N = 3 frames per view, frames [1, 3) of the left one, the rectangle (-7, -13, 64 x 64) of the 37 x 50 frame -- the whole padded image, so all
    four paddings are reached -- in both byte orders, into a poisoned plane 16 bytes into its allocation whose rows are 12 bytes wider than their
    pixels and whose frames lie 8 bytes apart.  The twin: 40 x 56 frames behind maps that reach over the frame's corners, constant border."""
    hw = (40, 56) if twin else (37, 50)
    frames, levels = views(layout, depth, align, 3, hw[1] + 5, 600, hw=hw, N=3)
    rectify, left_levels = None, levels[0]
    if twin:
        rectify = StereoRectifier(rotated_map(37, 50, 40, 56, 0.21, 1.2, "constant", 200), rotated_map(37, 50, 40, 56, -0.17, 1.25, "constant", 200))
        left_levels = remapped_levels(left_levels, rectify.left, depth)
    float_left = left_levels.float() if depth == 8 else as_float(left_levels, depth)          # frames.to_float(), rectified: the levels are the packer's
    with torch.cuda.device(DEV):
        source = stereo_source("colour test", *frames, rectify=rectify)
        assert source.size == (37, 50) and source.n == 3 and source._entry == "ppms_video_ingest_rgb_packed" + "_remap" * twin
        assert torch.equal(source.float_views()[0], float_left)
        for order in ("rgba8", "bgra8"):
            dest = ColourDest(2, 64, 64, pitch_extra=12, frame_gap=8, lead=16)
            source.colour(dest.plane, 1, 2, -7, -13, 64, 64, order)
            want = colour_bytes(padded_float(float_left[1:3], -7, -13, 64, 64), order)
            dest.check(want)
            assert len(want[..., :3].unique()) > 100 and bool((want[..., 3] == 255).all()) and not torch.equal(want[0], want[1])
    if not twin:
        assert torch.equal(float_left, frames[0].to_float())


# ---- the model: forward on interleaved frames is forward on the planar video ---------------------------------------------------------------------
def test_model_forward_on_the_halves_of_a_bgr_surface(model):
    """One (3, 64, 512, 3) BGR tensor of a stereo head, split: two views of 64 x 256 over one buffer."""
    hwc = rand_u8((3, 64, 512, 3), 610).to(DEV)
    left, right = PackedRGBFrames.from_hwc(hwc).split_side_by_side()
    assert left.data.data_ptr() == right.data.data_ptr() and (right.x0, right.width) == (256, 256)
    d, u = model.forward(left, right, iters=4, test_mode=True)
    rd, ru = model.forward(left.unpack()[None], right.unpack()[None], iters=4, test_mode=True)
    assert left.unpack().dtype == torch.uint8 and torch.equal(left.unpack(), hwc[:, :, :256].permute(0, 3, 1, 2)[:, [2, 1, 0]])
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.isfinite(d).all() and torch.equal(d, rd) and torch.equal(u, ru)
    with pytest.raises(ValueError):                              # the two views must be one kind of frame
        model.forward(left, PackedRGBFrames(right.data, 256, "rgb24", x0=256), iters=4, test_mode=True)
    with pytest.raises(TypeError):
        model.forward(left, right.unpack()[None], iters=4, test_mode=True)


def planar_video(hwc, pick):
    """(N, 2, H, W, C) uint8 -> the planar uint8 video (N, 2, 3, H, W) of its channels `pick` = (R, G, B)."""
    return hwc.permute(0, 1, 4, 2, 3)[:, :, list(pick)].contiguous()


def test_model_bgra_video_from_the_host_and_from_the_device(model):
    """A host (3, 2, 60, 250, 4) BGRA video -> 64 x 256, one window: the pixels' own 4 bytes are what crosses to the device."""
    hwc = rand_u8((3, 2, 60, 250, 4), 611)
    video = PackedRGBStereoVideo.from_hwc(hwc, "bgra")
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    ref = run(planar_video(hwc, (2, 1, 0)))
    out = run(video)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and torch.isfinite(out["disparity"]).all() and same(out, ref)
    on_device = video.to(DEV)
    assert on_device.left.data.is_cuda and on_device.left.data.dtype == torch.uint8 and tuple(on_device.left.data.shape) == (3, 60, 4 * 250)
    assert same(run(on_device), ref)


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    hwc = rand_u8((7, 2, 60, 250, 4), 612)
    assert len(window_plan(7, 4)) > 1
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2)
    out = run(PackedRGBStereoVideo.from_hwc(hwc, "bgra"))
    assert tuple(out["disparity"].shape) == (7, 1, 60, 250) and same(out, run(planar_video(hwc, (2, 1, 0))))


def x2rgb10_words(levels, seed):
    """levels (..., 3, H, W) int64 below 1024 -> int32 (..., H, W): R << 20 | G << 10 | B with random bits 30 and 31."""
    top = torch.randint(0, 4, levels[..., 0, :, :].shape, generator=torch.Generator().manual_seed(seed))
    w = levels[..., 0, :, :] << 20 | levels[..., 1, :, :] << 10 | levels[..., 2, :, :] | top << 30
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def test_model_x2rgb10_video_with_rectify_and_quantised_coloured_output(model):
    """Raw 70 x 262 x2rgb10 frames of an unrectified rig -> rectified 60 x 250, u16 disparity, u8 confidence and the bgra8 colour plane: the bytes of
    the same call on the float video of the rectified levels."""
    r = smooth_rectifier(60, 250, 70, 262, 8, "constant", 200)
    levels = torch.randint(0, 1024, (3, 2, 3, 70, 262), generator=torch.Generator().manual_seed(613))
    words = x2rgb10_words(levels, 614)
    video = PackedRGBStereoVideo(*(PackedRGBFrames(words[:, i].contiguous(), 262, "x2rgb10") for i in range(2)))
    assert torch.equal(video.left.unpack().long(), levels[:, 0]) and torch.equal(video.right.to_float(), as_float(levels[:, 1], 10))
    rect = torch.stack(r.apply_levels(video.left.unpack(), video.right.unpack(), 10), dim=1)
    assert tuple(rect.shape) == (3, 2, 3, 60, 250) and torch.equal(rect[:, 0].long(), remapped_levels(levels[:, 0], r.left, 10))
    spec = OutputSpec("u16", uncertainty="u8", colour="bgra8")
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, output=spec, **kw)
    q, qref = run(video, rectify=r), run(as_float(rect, 10))
    assert list(q) == list(qref) and {"disparity", "uncertainties", "colour"} <= set(q)
    assert q["disparity"].dtype == torch.uint16 and q["uncertainties"].dtype == torch.uint8 and tuple(q["colour"].shape) == (3, 60, 250, 4)
    for k in q:
        assert torch.equal(q[k].view(torch.uint8), qref[k].view(torch.uint8)), k
    assert torch.equal(q["colour"], colour_bytes(as_float(rect[:, 0], 10), "bgra8"))


def test_user_supplied_encoders_get_to_float():
    """Encoder callables of the caller (the stand-ins of stub_encoders.py, keyed on a frame's grey level): the deep video is converted on the device
    with to_float() and takes the float path.  Grey frames of level 4 f: 4 f * 255 / 1023 rounds to f."""
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()

    def grey(N, H0, W0):
        levels = (4 * torch.arange(N))[:, None, None, None].expand(N, 3, H0, W0)
        return PackedRGBStereoVideo(*(PackedRGBFrames(x2rgb10_words(levels, 615 + i), W0, "x2rgb10") for i in range(2)))

    video = grey(7, 60, 250)
    fl = torch.stack([video.left.to_float(), video.right.to_float()], dim=1)
    assert [round(float(x)) for x in fl[:, 0, 0, 0, 0]] == list(range(7)) and torch.equal(fl[:, 0, 1], as_float(4 * torch.arange(7), 10)[:, None, None].expand(7, 60, 250))
    run = lambda v: m.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    assert same(run(video), run(fl))
    v = grey(3, 64, 256).to(DEV)
    d, u = m.forward(v.left, v.right, iters=4, test_mode=True)
    rd, ru = m.forward(v.left.to_float()[None], v.right.to_float()[None], iters=4, test_mode=True)
    assert torch.equal(d, rd) and torch.equal(u, ru)
