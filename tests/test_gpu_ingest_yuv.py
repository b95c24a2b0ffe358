"""GPU: the decoded-video front door.  ppms_video_ingest_yuv420 on NV12 / I420 frames against ppms_video_ingest_u8 fed the RGB bytes that
this file's own restatement of the conversion (include/ppms.h) gives -- bit-exact, both bf16 planes as int16 -- and PPMStereo.forward /
forward_batch_test on YUVFrames / a YUVStereoVideo against the same calls on that RGB uint8 video (torch.equal)."""
import itertools

import pytest
import torch

from ppmstereo_amd.ppmstereo import YUVFrames, YUVStereoVideo
from ingest_util import DEV, bits, fresh, ingest, ingest_yuv, model, patterned, rand_u8, same  # noqa: F401  (model: the fixture)
from test_gpu_block import W

pytestmark = pytest.mark.gpu
COMBOS = list(itertools.product(("bt709", "bt601"), (False, True)))


# ---- the expectation: the conversion restated (not YUVFrames.to_rgb_u8), then the uint8 kernel -----------------------------------------
def restated_rgb(y, u, v, standard="bt709", full_range=False, shift=14):
    """y (N, H0, W0), u / v (N, ceil(H0/2), ceil(W0/2)) uint8 -> (N, 3, H0, W0) uint8 by the header's integer formula: coefficients rounded
    from doubles, every chroma sample repeated over its 2 x 2 luma pixels, floor division by 2^shift."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[standard]
    kg = 1.0 - kr - kb
    sy, sc, y_off = (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)
    one = 2.0 ** shift
    cy, crv, cbu = round(sy * one), round(sc * 2 * (1 - kr) * one), round(sc * 2 * (1 - kb) * one)
    cgu, cgv = round(sc * 2 * kb * (1 - kb) / kg * one), round(sc * 2 * kr * (1 - kr) / kg * one)
    H0, W0 = y.shape[1:]
    up = lambda c: c.long().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H0, :W0]
    d, e, f = y.long() - y_off, up(u) - 128, up(v) - 128
    half, div = 1 << (shift - 1), 1 << shift
    sums = torch.stack([cy * d + crv * f + half, cy * d - cgu * e - cgv * f + half, cy * d + cbu * e + half], dim=1)
    return torch.div(sums, div, rounding_mode="floor").clamp(0, 255).to(torch.uint8).contiguous()


def rgb_of(frames: YUVFrames):
    return restated_rgb(frames.y, frames.u, frames.v, frames.standard, frames.full_range)


def expected_operands(left: YUVFrames, right: YUVFrames, pad_left, pad_top, H, Wd):
    """The two operands ppms_video_ingest_u8 writes for the restated RGB bytes of both views."""
    l, r = rgb_of(left), rgb_of(right)
    N, _, H0, W0 = l.shape
    f, c = fresh(N, H, Wd)
    ingest(l.data_ptr(), r.data_ptr(), 3 * H0 * W0, N, H0, W0, pad_left, pad_top, H, Wd, f.view(), c.view())
    torch.cuda.synchronize()                                    # (l, r are released on return)
    return f, c


def check_both(left, right, pad_left, pad_top, H, Wd):
    ef, ec = expected_operands(left, right, pad_left, pad_top, H, Wd)
    f, c = fresh(left.n, H, Wd)
    ingest_yuv(left, right, pad_left, pad_top, H, Wd, f.view(), c.view())
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    return f, c


def nv12_surfaces(N, H0, W0, pitch, seed, **kw):
    """NV12 frames of H0 x W0 in surfaces whose rows are `pitch` bytes (luma and UV alike), on the device."""
    hc, wc = (H0 + 1) // 2, (W0 + 1) // 2
    y, uv = rand_u8((N, H0, pitch), seed).to(DEV), rand_u8((N, hc, pitch // 2, 2), seed + 100).to(DEV)
    return YUVFrames.nv12(y[:, :, :W0], uv[:, :, :wc], **kw)


def i420_planes(N, H0, W0, seed, **kw):
    hc, wc = (H0 + 1) // 2, (W0 + 1) // 2
    return YUVFrames.i420(rand_u8((N, H0, W0), seed).to(DEV), rand_u8((N, hc, wc), seed + 100).to(DEV), rand_u8((N, hc, wc), seed + 200).to(DEV), **kw)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def test_kernel_nv12_with_odd_sizes_and_padding():
    """37 x 50 per view in surfaces of pitch 64 (19 x 25 chroma samples, UV rows of 64 > 2 * 25 bytes) -> 64 x 64, pads 7 / 7 / 13 / 14."""
    from ppmstereo_amd.ppmstereo import InputPadder
    left, right = nv12_surfaces(2, 37, 50, 64, 31), nv12_surfaces(2, 37, 50, 64, 32)
    s = left.view_struct()
    assert (s.pitch_y, s.pitch_c, s.step_c, s.v - s.u, s.frame_stride_y, s.frame_stride_c) == (64, 64, 2, 1, 37 * 64, 19 * 64)
    padder = InputPadder((37, 50), divis_by=32)
    assert padder._pad == [7, 7, 13, 14]
    f, c = check_both(left, right, *padder.geometry())
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed


def test_kernel_i420_dense_planes_and_skipped_destinations():
    """Three dense planes per view, 32 x 64, T = 3, no padding; a destination with hi == NULL is skipped and stays as it was."""
    left, right = i420_planes(3, 32, 64, 33), i420_planes(3, 32, 64, 34)
    assert (left.pitch_y, left.pitch_c, left.step_c) == (64, 32, 1)
    ef, ec = expected_operands(left, right, 0, 0, 32, 64)
    for skip in ("cnet", "fnet"):
        f, c = patterned(6 * 16 * 32, 32), patterned(3 * 8 * 16, 64)
        before_f, before_c = bits(f).clone(), bits(c).clone()
        fv, cv = f.view(), c.view()
        if skip == "cnet":
            cv.hi = None                                         # (lo, ld, c stay set: hi == NULL alone must be enough to skip)
        else:
            fv.hi = None
        ingest_yuv(left, right, 0, 0, 32, 64, fv, cv)
        if skip == "cnet":
            assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), before_c)
        else:
            assert torch.equal(bits(c), bits(ec)) and torch.equal(bits(f), before_f)


@pytest.mark.parametrize("packing,shape", [("split_side_by_side", (2, 32, 128)), ("split_top_bottom", (2, 64, 64))])
def test_kernel_both_views_in_one_nv12_frame(packing, shape):
    """One decoded frame holds both views: the split helpers give two 32 x 64 views into the one surface."""
    N, Hp, Wp = shape
    y, uv = rand_u8(shape, 35).to(DEV), rand_u8((N, Hp // 2, Wp // 2, 2), 36).to(DEV)
    left, right = getattr(YUVFrames.nv12(y, uv), packing)()
    assert (left.height, left.width, right.height, right.width) == (32, 64, 32, 64)
    assert left.y.data_ptr() == y.data_ptr() and right.y.data_ptr() == y.data_ptr() + (64 if packing == "split_side_by_side" else 32 * 64)
    assert (right.pitch_y, right.frame_stride_y, right.step_c) == (Wp, Hp * Wp, 2)
    check_both(left, right, 0, 0, 32, 64)
    # and the views are the halves of the packed picture
    whole = restated_rgb(y, uv[..., 0], uv[..., 1])
    halves = (whole[..., :64], whole[..., 64:]) if packing == "split_side_by_side" else (whole[:, :, :32], whole[:, :, 32:])
    assert torch.equal(rgb_of(left), halves[0]) and torch.equal(rgb_of(right), halves[1])


def test_kernel_block_straddling_both_destinations():
    """36 x 36 from 33 x 35 with pads [1, 0, 2, 1]: the k = 2 part is 2592 threads, so one 256-thread block serves the end of one destination
    and the start of the other; the odd pad_left and the even pad_top shift the luma / chroma parity against the output's 2 x 2 phases."""
    left, right = i420_planes(1, 33, 35, 37), nv12_surfaces(1, 33, 35, 48, 38)
    assert (2 * 18 * 18 * 4) % 256
    check_both(left, right, 1, 2, 36, 36)
    check_both(right, left, 1, 1, 36, 36)                       # both pads odd: pad_top = 1 of the 3 spare rows


def test_kernel_frame_strides_past_2_to_31():
    """Frame 1 of every plane lies more than 2^31 bytes behind frame 0 (odd strides): the source offsets are 64-bit arithmetic.  One buffer
    for luma, one for both chroma planes (u at 0, v behind it), shared by the two views' (different) pictures at different offsets."""
    H0, W0, sy, sc = 8, 12, (1 << 31) + 4097, (1 << 31) + 4099
    ny, nc = H0 * W0, (H0 // 2) * (W0 // 2)
    ybuf = torch.empty(sy + 2 * ny, dtype=torch.uint8, device=DEV)
    cbuf = torch.empty(sc + 4 * nc, dtype=torch.uint8, device=DEV)
    views = []
    for i in range(2):                                          # view i: luma at i * ny, u at 2 i nc, v at (2 i + 1) nc
        src = i420_planes(2, H0, W0, 39 + i)
        y = torch.as_strided(ybuf, (2, H0, W0), (sy, W0, 1), i * ny)
        u, v = (torch.as_strided(cbuf, (2, H0 // 2, W0 // 2), (sc, W0 // 2, 1), (2 * i + j) * nc) for j in range(2))
        y.copy_(src.y), u.copy_(src.u), v.copy_(src.v)
        views.append(YUVFrames.i420(y, u, v))
        s = views[-1].view_struct()
        assert (s.frame_stride_y, s.frame_stride_c) == (sy, sc) and torch.equal(rgb_of(views[-1]), rgb_of(src))
    check_both(views[0], views[1], 0, 0, H0, W0)


def all_bytes_frame(seed, **kw):
    """One 32 x 32 frame: the Y plane holds every byte value four times, the 16 x 16 U and V planes every byte value once, each in its own
    order -- values below 16 and above 235 / 240 meet saturated chroma, so both clamps act."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randperm(1024, generator=g) % 256).to(torch.uint8).reshape(1, 32, 32)
    u, v = (torch.randperm(256, generator=g).to(torch.uint8).reshape(1, 16, 16) for _ in range(2))
    return YUVFrames.i420(y.to(DEV), u.to(DEV), v.to(DEV), **kw)


@pytest.mark.parametrize("standard,full_range", COMBOS)
def test_kernel_every_standard_and_range(standard, full_range):
    left, right = (all_bytes_frame(41 + i, standard=standard, full_range=full_range) for i in range(2))
    rgb = rgb_of(left)
    assert (rgb == 0).sum() > 8 and (rgb == 255).sum() > 8                                # (the clamps are reached)
    check_both(left, right, 0, 0, 32, 32)


@pytest.mark.parametrize("standard,full_range", COMBOS)
def test_to_rgb_u8_on_the_device_is_the_restatement(standard, full_range):
    kw = dict(standard=standard, full_range=full_range)
    for frames in (all_bytes_frame(43, **kw), nv12_surfaces(2, 37, 51, 64, 44, **kw), i420_planes(2, 33, 35, 45, **kw)):
        got = frames.to_rgb_u8()
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, rgb_of(frames))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def host_video(N, H0, W0, seed, nv12=True):
    """A YUVStereoVideo on the host (NV12 or I420 planes per view) and the (N, 2, 3, H0, W0) uint8 RGB video the restatement makes of it."""
    hc, wc = (H0 + 1) // 2, (W0 + 1) // 2
    views = []
    for i in range(2):
        y = rand_u8((N, H0, W0), seed + i)
        if nv12:
            views.append(YUVFrames.nv12(y, rand_u8((N, hc, wc, 2), seed + 10 + i)))
        else:
            views.append(YUVFrames.i420(y, rand_u8((N, hc, wc), seed + 10 + i), rand_u8((N, hc, wc), seed + 20 + i)))
    return YUVStereoVideo(*views), torch.stack([rgb_of(v) for v in views], dim=1).contiguous()


def test_model_single_window(model):
    """(3, 60, 250) frames -> 64 x 256, one window: the YUV video gives the bits of the uint8 RGB video, from the host and from the device."""
    video, rgb = host_video(3, 60, 250, 51)
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    ref, ref2 = run(rgb), run(rgb)
    assert same(ref, ref2), "the uint8 path itself is not repeatable: nothing can be said about the YUV path"
    out = run(video)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and not out["disparity"].is_cuda and out["disparity"].dtype == torch.float32
    assert torch.isfinite(out["disparity"]).all() and same(out, ref)
    on_device = video.to(DEV)
    assert on_device.left.y.is_cuda and on_device.left.step_c == 2 and torch.equal(rgb_of(on_device.right).cpu(), rgb[:, 1])
    assert same(run(on_device), ref)


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    video, rgb = host_video(7, 60, 250, 52, nv12=False)
    assert len(window_plan(7, 4)) > 1
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2)
    ref = run(rgb)
    out = run(video)
    assert tuple(out["disparity"].shape) == (7, 1, 60, 250) and same(out, ref)


def test_model_forward_directly(model):
    video, rgb = host_video(3, 64, 256, 53)
    left, right = video.left.to(DEV), video.right.to(DEV)
    d, u = model.forward(left, right, iters=4, test_mode=True)
    i1, i2 = rgb[None, :, 0].to(DEV), rgb[None, :, 1].to(DEV)
    rd, ru = model.forward(i1, i2, iters=4, test_mode=True)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.equal(d, rd) and torch.equal(u, ru)
    for a, b in ((left, i2), (i1, right), (left, i2.float())):
        with pytest.raises(TypeError):
            model.forward(a, b, iters=4, test_mode=True)


def test_user_supplied_encoders_get_the_converted_float_images():
    """Encoder callables of the caller (the stand-ins of stub_encoders.py, keyed on a frame's grey level): the YUV video is converted on the
    device and takes the float path.  Full-range grey frames: (Y, 128, 128) is the RGB grey Y."""
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet, frame_video
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()

    def grey(N, H0, W0):
        y = frame_video(N, H0, W0)[:, 0, 0].to(torch.uint8)
        c = torch.full((N, (H0 + 1) // 2, (W0 + 1) // 2), 128, dtype=torch.uint8)
        view = lambda: YUVFrames.i420(y.clone(), c.clone(), c.clone(), full_range=True)
        return YUVStereoVideo(view(), view())

    video = grey(7, 60, 250)
    rgb = torch.stack([rgb_of(video.left), rgb_of(video.right)], dim=1)
    assert torch.equal(rgb, frame_video(7, 60, 250).to(torch.uint8))
    run = lambda v: m.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    assert same(run(video), run(rgb))
    v = grey(3, 64, 256).to(DEV)
    d, u = m.forward(v.left, v.right, iters=4, test_mode=True)
    rd, ru = m.forward(rgb_of(v.left)[None], rgb_of(v.right)[None], iters=4, test_mode=True)
    assert torch.equal(d, rd) and torch.equal(u, ru)
