"""GPU: the raw-sensor front door.  ppms_video_ingest_raw (+ _remap) against the float path's own op chain (test_gpu_ingest_u8.float_path_operands)
fed ``RawFrames.to_float()`` -- whose levels tests/test_ingest_raw.py holds against a per-pixel restatement of the header's demosaic -- bit-exact,
both bf16 planes as int16; the remap also against test_gpu_ingest_yuv_deep's restatement of the blend; and PPMStereo.forward / forward_batch_test
on RawFrames / a RawStereoVideo against the same calls on that float video (torch.equal)."""
import pytest
import torch

from ppmstereo_amd.ppmstereo import OutputSpec, RawFrames, RawStereoVideo, RectifyMap, StereoRectifier
from ingest_util import DEV, bits, float_path_operands, fresh, ingest, ingest_raw, model, rand_u8, rand_u16, rotated_map, same  # noqa: F401  (model: the fixture)
from test_gpu_block import W
from test_gpu_ingest_yuv_deep import restated_remap_levels
from test_gpu_ingest_remap import smooth_rectifier

pytestmark = pytest.mark.gpu
PATTERNS = ["rggb", "bggr", "grbg", "gbrg", "mono"]
FORMATS = [(8, "lsb"), (10, "msb"), (12, "lsb")]                       # bytes; bits at the top, dirty below; bits at the bottom, dirty above


def raw_surface(N, H0, W0, pitch, seed, pattern, depth, align, **kw):
    """Raw frames of H0 x W0 in a device surface whose rows are `pitch` samples: every word random, so the unused bits of 16-bit words are dirty."""
    if depth == 8:
        surface = rand_u8((N, H0, pitch), seed).to(DEV)
    else:
        surface = rand_u16((N, H0, pitch), seed).to(DEV)
        unused = surface.to(torch.int32) & ((1 << (16 - depth)) - 1) if align == "msb" else surface.to(torch.int32) >> depth
        assert bool(unused.any())
    return RawFrames(surface[:, :, :W0], pattern, depth, align, **kw)


def float_video(frames: RawFrames, m: RectifyMap = None):
    """The float32 video the float door would be given: to_float(), or with a map the levels' remap (RectifyMap.apply_levels, held against the
    restated blend) and the tone curve behind it."""
    if m is None:
        return frames.to_float()
    levels = frames.to_rgb()
    rect = m.apply_levels(levels, frames.depth)
    assert torch.equal(rect.long(), restated_remap_levels(levels.long(), m, frames.depth))
    return frames.levels_to_float(rect)


def check_both(left, right, pad, maps=None):
    """pad = F.pad's [left, right, top, bottom]; maps: the two views' RectifyMaps (the _remap twin)."""
    fl, fr = (float_video(v, None if maps is None else maps[i]) for i, v in enumerate((left, right)))
    assert fl.dtype == torch.float32 and fl.is_cuda
    ef, ec, H, Wd = float_path_operands(fl, fr, pad)
    torch.cuda.synchronize()
    f, c = fresh(left.n, H, Wd)
    ingest_raw(left, right, pad[0], pad[2], H, Wd, f.view(), c.view(), maps)
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    return f, c


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,align", FORMATS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_plain_call_against_the_float_door(pattern, depth, align):
    """37 x 50 per view in surfaces of pitch 64 samples, two frames -> 64 x 64, pads 7 / 7 / 13 / 14: the padding clamps onto border pixels, whose
    neighbours are reflections."""
    from ppmstereo_amd.ppmstereo import InputPadder
    left, right = (raw_surface(2, 37, 50, 64, 171 + i, pattern, depth, align) for i in range(2))
    s = left.view_struct()
    assert (s.pitch, s.frame_stride) == (64 * left.sample_bytes, 37 * 64 * left.sample_bytes) and left.lsb == (6 if depth == 10 else 0)
    padder = InputPadder((37, 50), divis_by=32)
    assert padder._pad == [7, 7, 13, 14] and padder.geometry() == (7, 13, 64, 64)
    f, c = check_both(left, right, padder._pad)
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_2_x_2_frame_where_every_neighbour_is_a_reflection(pattern):
    """2 x 2 -> 4 x 4, one row and one column of padding all round, bytes and 12-bit words."""
    for depth, align in ((8, "lsb"), (12, "msb")):
        left, right = (raw_surface(2, 2, 2, 8, 175 + i, pattern, depth, align) for i in range(2))
        check_both(left, right, [1, 1, 1, 1])


def test_mono8_is_the_uint8_kernel_on_the_plane_repeated():
    """Unit gains, zero black, no tone curve: Mono8 37 x 50 (pitch 64) writes ppms_video_ingest_u8's operands for (plane, plane, plane)."""
    left, right = (raw_surface(2, 37, 50, 64, 177 + i, "mono", 8, "lsb") for i in range(2))
    l, r = (v.data[:, None].expand(2, 3, 37, 50).contiguous() for v in (left, right))
    ef, ec = fresh(2, 64, 64)
    ingest(l.data_ptr(), r.data_ptr(), 3 * 37 * 50, 2, 37, 50, 7, 13, 64, 64, ef.view(), ec.view())
    torch.cuda.synchronize()
    f, c = fresh(2, 64, 64)
    ingest_raw(left, right, 7, 13, 64, 64, f.view(), c.view())
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))


def test_skipped_destinations():
    """32 x 64, T = 3, no padding; a destination with hi == NULL is skipped and stays as it was."""
    left, right = (raw_surface(3, 32, 64, 64, 179 + i, "bggr", 10, "lsb") for i in range(2))
    ef, ec, H, Wd = float_path_operands(left.to_float(), right.to_float(), [0, 0, 0, 0])
    torch.cuda.synchronize()
    for skip in ("cnet", "fnet"):
        f, c = fresh(3, 32, 64)
        before_f, before_c = bits(f).clone(), bits(c).clone()
        fv, cv = f.view(), c.view()
        if skip == "cnet":
            cv.hi = None                                         # (lo, ld, c stay set: hi == NULL alone must be enough to skip)
        else:
            fv.hi = None
        ingest_raw(left, right, 0, 0, H, Wd, fv, cv)
        if skip == "cnet":
            assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), before_c)
        else:
            assert torch.equal(bits(c), bits(ec)) and torch.equal(bits(f), before_f)


@pytest.mark.parametrize("pattern,depth,align", [("grbg", 8, "lsb"), ("gbrg", 12, "msb")])
def test_a_block_straddling_both_destinations(pattern, depth, align):
    """36 x 36 from 33 x 35 with pads [1, 0, 2, 1]: the k = 2 part is 2592 threads, so one 256-thread block serves the end of one destination and
    the start of the other; the odd pad_left shifts the mosaic's parity against the output's 2 x 2 phases."""
    left, right = (raw_surface(1, 33, 35, 35, 181 + i, pattern, depth, align) for i in range(2))
    assert (2 * 18 * 18 * 4) % 256
    check_both(left, right, [1, 0, 2, 1])
    check_both(right, left, [1, 0, 1, 2])                       # both pads odd: pad_top = 1 of the 3 spare rows


def monotone_table(depth, seed):
    """2^depth sorted random values in [0, 255], both ends reached."""
    t = torch.rand(1 << depth, generator=torch.Generator().manual_seed(seed)).sort().values * 255.0
    t[0], t[-1] = 0.0, 255.0
    assert bool((t[1:] >= t[:-1]).all()) and len(set(t.tolist())) > (1 << depth) // 2
    return t


def test_tone_table_black_level_and_gains():
    """A random monotone tone curve through the kernel's table is the float door on to_float() = tone[levels]; with a black level and gains that
    send samples to both clamps."""
    tone = monotone_table(10, 183)
    kw = dict(black=70, gains=(1.93, 1.0, 1.52), tone=tone)
    left, right = (raw_surface(2, 37, 50, 64, 184 + i, "rggb", 10, "msb", **kw) for i in range(2))
    levels = left.to_rgb()
    assert int((levels == 0).sum()) > 50 and int((levels == 1023).sum()) > 50                # both ends of the table are looked up
    assert torch.equal(left.to_float(), tone.to(DEV)[levels.long()])
    lut = left.table(DEV)
    assert left.table(DEV) is lut and left[1:].table(DEV) is lut and right.table(DEV) is not lut          # built once per source object
    assert torch.equal(lut, 2 * (tone.to(DEV) / 255.0) - 1.0) and float(lut[0]) == -1.0 and float(lut[-1]) == 1.0
    check_both(left, right, [7, 7, 13, 14])
    plain = RawFrames(left.data, "rggb", 10, "msb", black=70, gains=(1.93, 1.0, 1.52))        # (without the curve: level_lut's table)
    from ppmstereo_amd.ppmstereo import level_lut
    assert plain.table(DEV) is level_lut(DEV, 10)
    check_both(plain, RawFrames(right.data, "rggb", 10, "msb", black=70, gains=(1.93, 1.0, 1.52)), [7, 7, 13, 14])


@pytest.mark.parametrize("tone", [False, True])
def test_every_level_of_a_12_bit_sensor(tone):
    """Mono12 64 x 64 frames holding each of the 4096 levels exactly once: every entry of the table is looked up, the last one included."""
    g = torch.Generator().manual_seed(186)
    planes = [torch.randperm(4096, generator=g).to(torch.int32).to(torch.uint16).reshape(1, 64, 64) for _ in range(2)]
    for p in planes:
        assert sorted(p.reshape(-1).to(torch.int32).tolist()) == list(range(4096))
    curve = monotone_table(12, 187) if tone else None
    left, right = (RawFrames(p.to(DEV), "mono", 12, tone=curve) for p in planes)
    assert torch.equal(left.to_rgb()[:, 0].to(torch.int32).cpu(), planes[0].to(torch.int32))
    check_both(left, right, [0, 0, 0, 0])
    bayer = [RawFrames(p.to(DEV), "bggr", 12, tone=curve) for p in planes]                  # and under a mosaic
    check_both(*bayer, [0, 0, 0, 0])


def test_frame_strides_past_2_to_31_bytes():
    """Frame 1 of each 16-bit view lies more than 2^31 bytes behind frame 0: the source offsets are 64-bit arithmetic.  One buffer, shared by the
    two views' (different) pictures at different offsets."""
    H0, W0, stride = 8, 12, (1 << 30) + 2049                                                  # in 16-bit elements
    n = H0 * W0
    buf = torch.empty(stride + 2 * n, dtype=torch.uint16, device=DEV)
    views = []
    for i in range(2):
        src = raw_surface(2, H0, W0, W0, 188 + i, "grbg", 12, "lsb", black=100, gains=(1.4, 1.0, 1.7))
        data = torch.as_strided(buf, (2, H0, W0), (stride, W0, 1), i * n)
        data.copy_(src.data)
        views.append(RawFrames(data, "grbg", 12, "lsb", black=100, gains=(1.4, 1.0, 1.7)))
        s = views[-1].view_struct()
        assert s.frame_stride == 2 * stride and 2 * stride > 1 << 31 and s.data == buf.data_ptr() + 2 * i * n
        assert torch.equal(views[-1].to_rgb(), src.to_rgb())
    check_both(views[0], views[1], [0, 0, 0, 0])


# ---- the _remap twin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,depth,align", [("rggb", 8, "lsb"), ("gbrg", 10, "msb"), ("mono", 12, "lsb")])
def test_remap_identity_maps_give_the_plain_calls_operands(pattern, depth, align):
    ident = RectifyMap.identity(37, 50, device=DEV)
    left, right = (raw_surface(2, 37, 50, 64, 190 + i, pattern, depth, align, black=3, gains=(1.2, 1.0, 1.1)) for i in range(2))
    ef, ec = fresh(2, 64, 64)
    ingest_raw(left, right, 7, 13, 64, 64, ef.view(), ec.view())
    f, c = check_both(left, right, [7, 7, 13, 14], (ident, ident))
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))


@pytest.mark.parametrize("border,fill", [("replicate", 0), ("constant", 0), ("constant", 255)])
def test_remap_rotated_scaled_map(border, fill):
    """Raw 40 x 56 frames (pitch 64) -> rectified 37 x 50 -> 64 x 64; the two views turn in opposite directions, and the maps' corners lie outside
    the raw frame.  A tap is demosaiced in the SOURCE frame: 10-bit Bayer words with a tone curve, and bytes."""
    lmap, rmap = rotated_map(37, 50, 40, 56, 0.21, 1.2, border, fill), rotated_map(37, 50, 40, 56, -0.17, 1.25, border, fill)
    assert lmap.view_struct(10).fill == (1023 if fill else 0)
    kw = dict(black=60, gains=(1.6, 1.0, 1.3), tone=monotone_table(10, 192))
    left, right = (raw_surface(2, 40, 56, 64, 193 + i, "bggr", 10, "msb", **kw) for i in range(2))
    check_both(left, right, [7, 7, 13, 14], (lmap, rmap))
    left, right = (raw_surface(2, 40, 56, 64, 195 + i, "grbg", 8, "lsb") for i in range(2))
    check_both(left, right, [7, 7, 13, 14], (lmap, rmap))


@pytest.mark.parametrize("border,fill", [("replicate", 0), ("constant", 255)])
def test_remap_a_map_that_points_far_outside_the_frame(border, fill):
    """Every tap of rectified row r lies far outside the 9 x 11 raw frame, in one of the four directions, the int16 extremes included: the result is
    the fill level, or the level of the corner pixel the taps are clamped onto -- never anything else."""
    hs, ws, H0, W0 = 9, 11, 8, 8
    far = torch.tensor([[-32768, -32768], [32767, -300], [-300, 32767], [32767, 32767], [-2, -2], [ws, hs], [20000, -20000], [-1000, 4]], dtype=torch.int16)
    xy = far[:, None, :].expand(H0, W0, 2).contiguous()
    frac = torch.full((H0, W0), 0x155, dtype=torch.int16)
    m = RectifyMap(xy, frac, (hs, ws), border, fill).to(DEV)
    left, right = (raw_surface(2, hs, ws, 16, 197 + i, "rggb", 12, "lsb", black=10, gains=(1.1, 1.0, 1.2)) for i in range(2))
    levels = left.to_rgb()
    got = m.apply_levels(levels, 12)
    corner = lambda y, x: levels[:, :, y, x][:, :, None].expand(2, 3, W0)
    if border == "constant":
        assert bool((got == 4095).all())                        # (row 7 too: its taps lie left of the frame)
    else:
        for row, (y, x) in enumerate([(0, 0), (0, ws - 1), (hs - 1, 0), (hs - 1, ws - 1), (0, 0), (hs - 1, ws - 1), (0, ws - 1)]):
            assert torch.equal(got[:, :, row], corner(y, x))
    check_both(left, right, [0, 0, 0, 0], (m, m))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def host_raw(N, H0, W0, seed, pattern="rggb", depth=10, align="msb", **kw):
    """A RawStereoVideo on the host (every word random) and the (N, 2, 3, H0, W0) float video of its to_float() frames."""
    plane = lambda s: rand_u8((N, H0, W0), s) if depth == 8 else rand_u16((N, H0, W0), s)
    views = [RawFrames(plane(seed + i), pattern, depth, align, **kw) for i in range(2)]
    return RawStereoVideo(*views), torch.stack([v.to_float() for v in views], dim=1).contiguous()


def test_model_single_window(model):
    """(3, 60, 250) BayerRG10 frames -> 64 x 256, one window: the bits of the float video of to_float(), from the host and from the device."""
    video, fl = host_raw(3, 60, 250, 201, black=64, gains=(1.7, 1.0, 1.4), tone=monotone_table(10, 202))
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    ref, ref2 = run(fl), run(fl)
    assert same(ref, ref2), "the float path itself is not repeatable: nothing can be said about the raw path"
    out = run(video)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and not out["disparity"].is_cuda and out["disparity"].dtype == torch.float32
    assert torch.isfinite(out["disparity"]).all() and same(out, ref)
    on_device = video.to(DEV)
    assert on_device.left.data.is_cuda and on_device.left.data.dtype == torch.uint16 and on_device.left.tone is video.left.tone
    assert same(run(on_device), ref)


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    video, fl = host_raw(7, 60, 250, 203, "gbrg", 8, "lsb", black=9, gains=(1.3, 1.0, 1.9))
    assert len(window_plan(7, 4)) > 1
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2)
    out = run(video)
    assert tuple(out["disparity"].shape) == (7, 1, 60, 250) and same(out, run(fl))


def test_model_forward_directly(model):
    video, fl = host_raw(3, 64, 256, 204, "mono", 12, "lsb", black=200)
    left, right = video.left.to(DEV), video.right.to(DEV)
    d, u = model.forward(left, right, iters=4, test_mode=True)
    fl = fl.to(DEV)
    rd, ru = model.forward(fl[None, :, 0], fl[None, :, 1], iters=4, test_mode=True)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.equal(d, rd) and torch.equal(u, ru)
    with pytest.raises(ValueError):                              # the two views must be one kind of frame
        model.forward(left, RawFrames(right.data, "mono", 12, "lsb", black=201), iters=4, test_mode=True)
    with pytest.raises(TypeError):
        model.forward(left, fl[None, :, 1], iters=4, test_mode=True)


def test_model_rectify_and_quantised_output(model):
    """Raw 70 x 262 Bayer frames -> rectified 60 x 250: rectify= gives the bits of the float video made with apply_levels and the tone curve behind
    it (float_views); output= those of the same call on the float video."""
    from ppmstereo_amd.video import stereo_source
    r = smooth_rectifier(60, 250, 70, 262, 7, "constant", 200)
    video, _ = host_raw(3, 70, 262, 205, "grbg", 10, "lsb", black=64, gains=(1.5, 1.0, 1.8), tone=monotone_table(10, 206))
    rect = torch.stack(stereo_source("test", video, rectify=r).float_views(), dim=1)
    assert tuple(rect.shape) == (3, 2, 3, 60, 250) and rect.dtype == torch.float32
    assert torch.equal(rect[:, 1], float_video(video.right.to(DEV), r.right.to(DEV)).cpu())
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, **kw)
    assert same(run(video, rectify=r), run(rect))
    plain, fl = host_raw(3, 60, 250, 207, "bggr", 12, "msb", black=256)
    spec = OutputSpec(disparity="u16", uncertainty="u8")
    q, qref = run(plain, output=spec), run(fl, output=spec)
    assert q["disparity"].dtype == torch.uint16 and q["uncertainties"].dtype == torch.uint8 and tuple(q["disparity"].shape) == (3, 1, 60, 250)
    for k in ("disparity", "uncertainties"):
        assert torch.equal(q[k].view(torch.uint8), qref[k].view(torch.uint8))


def test_user_supplied_encoders_get_float_views():
    """Encoder callables of the caller (the stand-ins of stub_encoders.py, keyed on a frame's grey level): the raw video is demosaiced (and
    rectified) on the device with to_rgb() / apply_levels and takes the float path.  A mosaic whose every site holds f is the grey f."""
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet, frame_video
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()

    def grey(N, H0, W0):
        plane = torch.arange(N, dtype=torch.uint8)[:, None, None].expand(N, H0, W0).contiguous()
        return RawStereoVideo(RawFrames(plane, "rggb"), RawFrames(plane.clone(), "rggb"))

    video = grey(7, 60, 250)
    fl = torch.stack([video.left.to_float(), video.right.to_float()], dim=1)
    assert torch.equal(fl, frame_video(7, 60, 250))
    run = lambda v, **kw: m.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, **kw)
    ref = run(fl)
    assert same(run(video), ref)
    r = smooth_rectifier(60, 250, 70, 262, 8)                   # replicate border: a constant frame stays that constant
    assert same(run(grey(7, 70, 262), rectify=r), ref)
    v = grey(3, 64, 256).to(DEV)
    d, u = m.forward(v.left, v.right, iters=4, test_mode=True)
    rd, ru = m.forward(v.left.to_float()[None], v.right.to_float()[None], iters=4, test_mode=True)
    assert torch.equal(d, rd) and torch.equal(u, ru)
