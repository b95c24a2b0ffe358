"""GPU: rectification inside the ingest kernel.  ppms_video_ingest_u8_remap / ppms_video_ingest_yuv420_remap on the raw frames of an unrectified
rig against ppms_video_ingest_u8 fed the rectified bytes that the tests' own restatement of the remap (tests/test_ingest_remap.py, not
RectifyMap.apply_u8) makes of them -- bit-exact, both bf16 planes as int16 -- and PPMStereo.forward / forward_batch_test with rectify= against
the same calls on that rectified uint8 video (torch.equal)."""
import pytest
import torch

from ppmstereo_amd.ppmstereo import OutputSpec, RectifyMap, StereoRectifier, YUVFrames, YUVStereoVideo
from ingest_util import DEV, bits, fresh, ingest, ingest_yuv, model, rand_u8, restated_remap, same  # noqa: F401  (model: the fixture)
from test_gpu_block import W
from test_gpu_ingest_yuv import COMBOS, i420_planes, nv12_surfaces, rgb_of
from test_ingest_remap import random_map

pytestmark = pytest.mark.gpu
BORDERS = [("replicate", 0), ("constant", 0), ("constant", 200)]


# ---- the expectation: the remap restated, then the uint8 kernel -----------------------------------------------------------------------------
def device_map(H0, W0, hs, ws, seed, border="replicate", fill=0, pitch=None):
    xy, frac = random_map(H0, W0, hs, ws, seed, pitch)
    xy_d, frac_d = xy.to(DEV), frac.to(DEV)
    if pitch:                                                   # rows of `pitch` map pixels on the device too
        full_xy, full_frac = torch.zeros((H0, pitch, 2), dtype=torch.int16, device=DEV), torch.zeros((H0, pitch), dtype=torch.int16, device=DEV)
        full_xy[:, :W0], full_frac[:, :W0] = xy_d, frac_d
        xy_d, frac_d = full_xy[:, :W0], full_frac[:, :W0]
    return RectifyMap(xy_d, frac_d, (hs, ws), border, fill)


def rectified(rgb, m: RectifyMap):
    return restated_remap(rgb, m.xy, m.frac, m.border, m.fill).contiguous()


def expected_operands(l_rect, r_rect, pad_left, pad_top, H, Wd):
    """The two operands ppms_video_ingest_u8 writes for rectified bytes (N, 3, H0, W0) of both views."""
    N, _, H0, W0 = l_rect.shape
    f, c = fresh(N, H, Wd)
    ingest(l_rect.data_ptr(), r_rect.data_ptr(), 3 * H0 * W0, N, H0, W0, pad_left, pad_top, H, Wd, f.view(), c.view())
    torch.cuda.synchronize()
    return f, c


def ingest_u8_remap(left, right, lmap: RectifyMap, rmap: RectifyMap, pad_left, pad_top, H, Wd, fview, cview):
    """left / right: raw (N, 3, hs, ws) uint8 on the device."""
    N, _, hs, ws = left.shape
    return ingest(left.data_ptr(), right.data_ptr(), 3 * hs * ws, N, None, None, pad_left, pad_top, H, Wd, fview, cview, (lmap, rmap))


def ingest_yuv_remap(left: YUVFrames, right: YUVFrames, lmap: RectifyMap, rmap: RectifyMap, pad_left, pad_top, H, Wd, fview, cview):
    return ingest_yuv(left, right, pad_left, pad_top, H, Wd, fview, cview, (lmap, rmap))


def check_u8(left, right, lmap, rmap, pad_left, pad_top, H, Wd):
    ef, ec = expected_operands(rectified(left, lmap), rectified(right, rmap), pad_left, pad_top, H, Wd)
    f, c = fresh(left.shape[0], H, Wd)
    assert ingest_u8_remap(left, right, lmap, rmap, pad_left, pad_top, H, Wd, f.view(), c.view()) == 0
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    return f, c


def check_yuv(left, right, lmap, rmap, pad_left, pad_top, H, Wd):
    ef, ec = expected_operands(rectified(rgb_of(left), lmap), rectified(rgb_of(right), rmap), pad_left, pad_top, H, Wd)
    f, c = fresh(left.n, H, Wd)
    assert ingest_yuv_remap(left, right, lmap, rmap, pad_left, pad_top, H, Wd, f.view(), c.view()) == 0
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    return f, c


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
def test_identity_maps_give_the_existing_kernels_operands():
    """37 x 50 -> 64 x 64 (pads 7 / 7 / 13 / 14): with identity maps _u8_remap writes ppms_video_ingest_u8's operands, and _yuv420_remap on NV12
    frames in pitch-64 surfaces ppms_video_ingest_yuv420's."""
    from ppmstereo_amd.ppmstereo import InputPadder
    ident = RectifyMap.identity(37, 50, device=DEV)
    geometry = InputPadder((37, 50), divis_by=32).geometry()
    assert geometry == (7, 13, 64, 64)
    left, right = rand_u8((2, 3, 37, 50), 61).to(DEV), rand_u8((2, 3, 37, 50), 62).to(DEV)
    assert torch.equal(rectified(left, ident), left)
    ef, ec = expected_operands(left, right, *geometry)
    f, c = check_u8(left, right, ident, ident, *geometry)
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed
    yl, yr = nv12_surfaces(2, 37, 50, 64, 63), nv12_surfaces(2, 37, 50, 64, 64)
    assert (yl.pitch_y, yl.pitch_c, yl.step_c) == (64, 64, 2)
    ef, ec = fresh(2, 64, 64)
    ingest_yuv(yl, yr, *geometry, ef.view(), ec.view())
    f, c = check_yuv(yl, yr, ident, ident, *geometry)
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))


@pytest.mark.parametrize("border,fill", BORDERS)
def test_random_maps_with_another_source_size(border, fill):
    """Source 41 x 53, rectified 37 x 50, padded to 64 x 64, two frames; x0 in [-3, ws + 2] and y0 in [-3, hs + 2] cross both borders, every one of
    the 1024 frac values occurs, the map rows have pitch 56, and the two views have different maps."""
    lmap, rmap = device_map(37, 50, 41, 53, 65, border, fill, pitch=56), device_map(37, 50, 41, 53, 66, border, fill, pitch=56)
    for m in (lmap, rmap):
        assert m.pitch == 56 and m.view_struct().pitch == 56 and not m.xy.is_contiguous()
        assert len(set(m.frac.reshape(-1).tolist())) == 1024
        assert (int(m.xy[..., 0].min()), int(m.xy[..., 0].max()), int(m.xy[..., 1].min()), int(m.xy[..., 1].max())) == (-3, 55, -3, 43)
    assert not torch.equal(lmap.xy, rmap.xy) and not torch.equal(lmap.frac, rmap.frac)
    left, right = rand_u8((2, 3, 41, 53), 67).to(DEV), rand_u8((2, 3, 41, 53), 68).to(DEV)
    check_u8(left, right, lmap, rmap, 7, 13, 64, 64)
    if border == "constant":                                    # one mode per view in one launch
        check_u8(left, right, lmap, RectifyMap(rmap.xy, rmap.frac, (41, 53), "replicate"), 7, 13, 64, 64)


@pytest.mark.parametrize("border,fill", [("replicate", 0), ("constant", 200)])
def test_int16_extremes(border, fill):
    """xy entries of -32768 and 32767 (with the largest fractions) in a 32 x 32 map: the tap coordinate x0 + 1 = 32768 is 32-bit arithmetic, every
    address is clamped into the 33 x 35 source, the call returns 0 and the result is the restatement's."""
    xy, frac = random_map(32, 32, 33, 35, 69)
    flat = xy.reshape(-1, 2)
    flat[0::7, 0], flat[1::7, 1], flat[2::7, 0], flat[3::7, 1] = -32768, -32768, 32767, 32767
    flat[4::7] = torch.tensor([32767, 32767], dtype=torch.int16)
    flat[5::7] = torch.tensor([-32768, -32768], dtype=torch.int16)
    frac.reshape(-1)[4::7] = 1023
    assert int(xy.min()) == -32768 and int(xy.max()) == 32767
    m = RectifyMap(xy.to(DEV), frac.to(DEV), (33, 35), border, fill)
    left, right = rand_u8((1, 3, 33, 35), 70).to(DEV), rand_u8((1, 3, 33, 35), 71).to(DEV)
    check_u8(left, right, m, m, 0, 0, 32, 32)
    check_yuv(i420_planes(1, 33, 35, 72), nv12_surfaces(1, 33, 35, 48, 73), m, m, 0, 0, 32, 32)
    torch.cuda.synchronize()


@pytest.mark.parametrize("standard,full_range", COMBOS)
def test_yuv_sources_with_odd_sizes_and_a_straddling_block(standard, full_range):
    """I420 (left) and NV12 in pitch-48 surfaces (right), odd 33 x 35 source, rectified 36 x 36 without padding: the k = 2 part is 2592 threads,
    so one 256-thread block serves the end of one destination and the start of the other."""
    kw = dict(standard=standard, full_range=full_range)
    left, right = i420_planes(1, 33, 35, 74, **kw), nv12_surfaces(1, 33, 35, 48, 75, **kw)
    assert (2 * 18 * 18 * 4) % 256
    lmap, rmap = device_map(36, 36, 33, 35, 76, "constant", 200), device_map(36, 36, 33, 35, 77)
    check_yuv(left, right, lmap, rmap, 0, 0, 36, 36)
    check_yuv(right, left, rmap, lmap, 0, 0, 36, 36)


def test_a_skipped_destination_stays_as_it_was():
    lmap, rmap = device_map(32, 64, 41, 53, 78, "constant", 9), device_map(32, 64, 41, 53, 79)
    left, right = rand_u8((3, 3, 41, 53), 80).to(DEV), rand_u8((3, 3, 41, 53), 81).to(DEV)
    ef, ec = expected_operands(rectified(left, lmap), rectified(right, rmap), 0, 0, 32, 64)
    for skip in ("cnet", "fnet"):
        f, c = fresh(3, 32, 64)
        before_f, before_c = bits(f).clone(), bits(c).clone()
        fv, cv = f.view(), c.view()
        if skip == "cnet":
            cv.hi = None                                         # (lo, ld, c stay set: hi == NULL alone must be enough to skip)
        else:
            fv.hi = None
        ingest_u8_remap(left, right, lmap, rmap, 0, 0, 32, 64, fv, cv)
        if skip == "cnet":
            assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), before_c)
        else:
            assert torch.equal(bits(c), bits(ec)) and torch.equal(bits(f), before_f)


@pytest.mark.parametrize("border,fill", BORDERS)
def test_apply_u8_on_the_device_is_the_restatement(border, fill):
    m = device_map(37, 50, 41, 53, 82, border, fill, pitch=56)
    rgb = rand_u8((2, 3, 41, 53), 83).to(DEV)
    got = m.apply_u8(rgb)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, rectified(rgb, m))
    host = RectifyMap(m.xy.cpu(), m.frac.cpu(), (41, 53), border, fill)      # a host map is moved once and kept
    assert torch.equal(host.apply_u8(rgb), got) and host.to(DEV) is host.to(DEV) and host.to(DEV).xy.is_cuda


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def smooth_rectifier(H0, W0, hs, ws, seed, border="replicate", fill=0) -> StereoRectifier:
    """Identity plus a low-amplitude warp (a few pixels), centred in the larger source frame; distinct per view.  On the host."""
    ys, xs = torch.meshgrid(torch.arange(H0, dtype=torch.float32), torch.arange(W0, dtype=torch.float32), indexing="ij")
    maps = []
    for i in range(2):
        a, b = 1.7 + 0.6 * i + 0.01 * seed, 1.1 + 0.4 * i
        mx = xs + (ws - W0) / 2 + a * torch.sin(ys / (11.0 + i) + 0.3 * seed) + 0.5 * torch.cos(xs / 23.0)
        my = ys + (hs - H0) / 2 + b * torch.cos(xs / (17.0 - i) + 0.2 * seed) + 0.003 * (xs - W0 / 2) * (1 - 2 * i)
        maps.append(RectifyMap.from_float(mx, my, (hs, ws), border, fill))
    assert not torch.equal(maps[0].xy, maps[1].xy) and len(set(maps[0].frac.reshape(-1).tolist())) > 500
    return StereoRectifier(*maps)


def raw_video(N, hs, ws, seed, nv12=True):
    """A raw YUVStereoVideo on the host, the (N, 2, 3, hs, ws) uint8 RGB video of its frames (test_gpu_ingest_yuv's restated conversion)."""
    hc, wc = (hs + 1) // 2, (ws + 1) // 2
    views = []
    for i in range(2):
        y = rand_u8((N, hs, ws), seed + i)
        if nv12:
            views.append(YUVFrames.nv12(y, rand_u8((N, hc, wc, 2), seed + 10 + i)))
        else:
            views.append(YUVFrames.i420(y, rand_u8((N, hc, wc), seed + 10 + i), rand_u8((N, hc, wc), seed + 20 + i)))
    return YUVStereoVideo(*views), torch.stack([rgb_of(v) for v in views], dim=1).contiguous()


def rectified_video(rgb, r: StereoRectifier):
    """(N, 2, 3, hs, ws) uint8 -> the (N, 2, 3, H0, W0) uint8 video a caller's own remap pass would hand to the uint8 front door."""
    return torch.stack([rectified(rgb[:, 0], r.left), rectified(rgb[:, 1], r.right)], dim=1).contiguous()


def test_model_single_window(model):
    """Raw 70 x 262 -> rectified 60 x 250 -> padded 64 x 256, one window: rectify= on the raw bytes gives the bits of the rectified uint8 video,
    from the host and from the device, for a uint8 tensor and for a YUVStereoVideo."""
    r = smooth_rectifier(60, 250, 70, 262, 1)
    yuv, rgb = raw_video(3, 70, 262, 91)
    rect = rectified_video(rgb, r)
    assert tuple(rect.shape) == (3, 2, 3, 60, 250)
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, **kw)
    ref, ref2 = run(rect), run(rect)
    assert same(ref, ref2), "the uint8 path itself is not repeatable: nothing can be said about the remap path"
    out = run(rgb, rectify=r)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and not out["disparity"].is_cuda and out["disparity"].dtype == torch.float32
    assert torch.isfinite(out["disparity"]).all() and same(out, ref)
    assert same(run(rgb.to(DEV), rectify=r), ref)
    assert same(run(yuv, rectify=r), ref)
    assert same(run(yuv.to(DEV), rectify=r.to(DEV)), ref)
    assert r.to(DEV).left is r.to(DEV).left and r.to(DEV).right.xy.is_cuda      # the maps crossed once and are kept


def test_model_several_windows_and_quantised_output(model):
    from ppmstereo_amd.ppmstereo import window_plan
    r = smooth_rectifier(60, 250, 70, 262, 2, "constant", 128)
    yuv, rgb = raw_video(7, 70, 262, 92, nv12=False)
    rect = rectified_video(rgb, r)
    assert len(window_plan(7, 4)) > 1
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2, **kw)
    ref = run(rect)
    out = run(rgb, rectify=r)
    assert tuple(out["disparity"].shape) == (7, 1, 60, 250) and same(out, ref)
    assert same(run(yuv, rectify=r), ref)
    spec = OutputSpec(disparity="u16", uncertainty="u8")
    qref, q = run(rect, output=spec), run(rgb, rectify=r, output=spec)
    assert q["disparity"].dtype == torch.uint16 and q["uncertainties"].dtype == torch.uint8 and tuple(q["disparity"].shape) == (7, 1, 60, 250)
    for k in ("disparity", "uncertainties"):
        assert torch.equal(q[k].view(torch.uint8), qref[k].view(torch.uint8))
    qy = run(yuv, rectify=r, output=spec)
    assert torch.equal(qy["disparity"].view(torch.uint8), qref["disparity"].view(torch.uint8)) and torch.equal(qy["uncertainties"], qref["uncertainties"])


def test_model_forward_directly(model):
    """Rectified 64 x 256 from a 72 x 270 source."""
    r = smooth_rectifier(64, 256, 72, 270, 3)
    yuv, rgb = raw_video(3, 72, 270, 93)
    rect = rectified_video(rgb, r).to(DEV)
    rd, ru = model.forward(rect[None, :, 0], rect[None, :, 1], iters=4, test_mode=True)
    raw = rgb.to(DEV)
    d, u = model.forward(raw[None, :, 0], raw[None, :, 1], iters=4, test_mode=True, rectify=r)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.equal(d, rd) and torch.equal(u, ru)
    d, u = model.forward(yuv.left.to(DEV), yuv.right.to(DEV), iters=4, test_mode=True, rectify=r)
    assert torch.equal(d, rd) and torch.equal(u, ru)
    with pytest.raises(TypeError):
        model.forward(raw[None, :, 0].float(), raw[None, :, 1].float(), iters=4, test_mode=True, rectify=r)
    with pytest.raises(ValueError):
        model.forward(rect[None, :, 0], rect[None, :, 1], iters=4, test_mode=True, rectify=r)     # already 64 x 256: not the maps' source size
    with pytest.raises(NotImplementedError):
        model.forward(raw[None, :, 0].expand(2, -1, -1, -1, -1), raw[None, :, 1].expand(2, -1, -1, -1, -1), iters=4, test_mode=True, rectify=r)


def test_user_supplied_encoders_take_the_apply_u8_fallback():
    """Encoder callables of the caller (the stand-ins of stub_encoders.py, keyed on a frame's grey level): the raw frames are rectified on the
    device with RectifyMap.apply_u8 and take the float path.  A constant frame stays that constant under a replicate-border remap."""
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet, frame_video
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()
    r = smooth_rectifier(60, 250, 70, 262, 4)
    raw = frame_video(7, 70, 262).to(torch.uint8)
    rect = rectified_video(raw, r)
    assert torch.equal(rect, frame_video(7, 60, 250).to(torch.uint8))
    run = lambda v, **kw: m.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, **kw)
    ref = run(rect)
    assert same(run(raw, rectify=r), ref)
    grey = lambda: YUVFrames.i420(raw[:, 0, 0].clone(), torch.full((7, 35, 131), 128, dtype=torch.uint8), torch.full((7, 35, 131), 128, dtype=torch.uint8),
                                  full_range=True)
    assert same(run(YUVStereoVideo(grey(), grey()), rectify=r), ref)
    r2 = smooth_rectifier(64, 256, 72, 270, 5)
    v = frame_video(3, 72, 270).to(torch.uint8).to(DEV)
    d, u = m.forward(v[None, :, 0], v[None, :, 1], iters=4, test_mode=True, rectify=r2)
    w = frame_video(3, 64, 256).to(torch.uint8).to(DEV)
    rd, ru = m.forward(w[None, :, 0], w[None, :, 1], iters=4, test_mode=True)
    assert torch.equal(d, rd) and torch.equal(u, ru)
