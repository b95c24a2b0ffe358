"""GPU: the quantised back door.  ppms_disparity_egress on synthetic engine state against OutputSpec.reference applied to ppms_bilinear's
output and the sliced flow_up, and PPMStereo.forward / forward_batch_test with output= against the reference applied to the default call's
float32 results.  Every comparison is exact: the kernel's steps are single fp32 operations rounded to nearest even, the reference's too
(NaN compares equal to NaN at the same place; its payload is not part of the definition)."""
import ctypes

import pytest
import torch

from ppmstereo_amd import _lib as L
from ppmstereo_amd import weights as Wm
from ppmstereo_amd.engine import bilinear
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_block import DEV, W

pytestmark = pytest.mark.gpu
FMT = {"f32": (L.FMT_F32, torch.float32, 4), "f16": (L.FMT_F16, torch.float16, 2), "u16": (L.FMT_U16, torch.uint16, 2), "u8": (L.FMT_U8, torch.uint8, 1)}
KEYS = ("disparity", "depth", "uncertainties")


def same(a, b):
    """Equal dtype, shape and values; NaN equals NaN."""
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        return False
    if a.dtype.is_floating_point:
        a, b = (torch.where(x.isnan(), torch.full_like(x, -1.0), x) for x in (a, b))
        return torch.equal(a, b)
    return torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a, b.view(torch.int16) if b.dtype == torch.uint16 else b)


def engine_state(T, H, Wd, seed, min_disp=0.25):
    """flow_up (T, 2, H, W): channel 0 = magnitudes in [0, 400) with both signs, exact zeros, values below min_disp, NaN and exact u16 ties k / 512
    sprinkled in; channel 1 = another pattern (a wrong channel stride shows).  unc (T, H/4, W/4) in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    n = T * H * Wd
    d = torch.rand(n, generator=g) * 400.0
    d = d * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    pick = torch.randperm(n, generator=g)
    q = n // 16
    d[pick[:q]] = 0.0
    d[pick[q:2 * q]] = torch.rand(q, generator=g) * min_disp * torch.where(torch.rand(q, generator=g) < 0.5, -1.0, 1.0)
    d[pick[2 * q:3 * q]] = float("nan")
    d[pick[3 * q:4 * q]] = (2 * torch.randint(0, 60000, (q,), generator=g) + 1).float() / 512.0 * torch.where(torch.rand(q, generator=g) < 0.5, -1.0, 1.0)
    flow = torch.stack([d.reshape(T, H, Wd), 1000.0 + torch.rand(T, H, Wd, generator=g)], dim=1).contiguous()
    unc = torch.rand(T, H // 4, Wd // 4, generator=g)
    return flow.to(DEV), unc.to(DEV)


def expected(spec, flow, unc, f0, f1, left, top, h0, w0):
    """OutputSpec.reference on the sliced flow_up and on ppms_bilinear's 4x upsampling of unc -- evaluated on the host, where torch's fp32
    division and conversions are the IEEE ones beyond doubt -> CPU tensors."""
    T, _, H, Wd = flow.shape
    up = bilinear(unc.view(T, 1, H // 4, Wd // 4), (H, Wd), False)
    cut = lambda x: x[f0:f1, :1, top:top + h0, left:left + w0].cpu()
    return spec.reference(cut(flow), cut(up))


class Dest:
    """A byte buffer of ``frames`` output frames with a pitch, filled with a non-zero pattern; the launch writes n frames from frame ``first`` on."""

    def __init__(self, fmt, frames, h0, w0, pitch_extra=0, first=0, frame_gap=0):
        self.fmt, self.h0, self.w0, self.first = fmt, h0, w0, first
        self.es = FMT[fmt][2]
        self.pitch = w0 * self.es + pitch_extra
        self.frame_stride = h0 * self.pitch + frame_gap
        size = frames * self.frame_stride
        self.pattern = (torch.arange(size, device=DEV) % 251 + 1).to(torch.uint8)
        self.buf = self.pattern.clone()

    def plane(self):
        return L.EgressPlane(self.buf.data_ptr() + self.first * self.frame_stride, self.frame_stride, self.pitch, FMT[self.fmt][0], 0)

    def region(self, t, n):
        return torch.as_strided(t, (n, self.h0, self.w0 * self.es), (self.frame_stride, self.pitch, 1), self.first * self.frame_stride)

    def written(self, n):
        """(n, 1, h0, w0) tensor of the plane's dtype: what lies in the n frames' rows."""
        return self.region(self.buf, n).contiguous().view(FMT[self.fmt][1]).reshape(n, 1, self.h0, self.w0).cpu()

    def rest_untouched(self, n):
        """Every byte outside the n frames' rows -- between rows, between frames, the frames before and after -- still holds the pattern."""
        mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.region(mask, n).fill_(True)
        return torch.equal(self.buf[~mask], self.pattern[~mask])

    def untouched(self):
        return torch.equal(self.buf, self.pattern)


NO_PLANE = L.EgressPlane(None, 0, 0, 0, 0)


def launch(flow, unc, f0, n, left, top, h0, w0, spec, dests):
    """dests: {key: Dest or None}"""
    T, _, H, Wd = flow.shape
    pl = [dests[k].plane() if dests.get(k) is not None else NO_PLANE for k in KEYS]
    out = L.Egress(pl[0], pl[1], pl[2], spec.disp_scale, spec.fb, spec.depth_scale, spec.min_disp)
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_disparity_egress(flow.data_ptr(), unc.data_ptr(), T, H, Wd, f0, n, left, top, h0, w0, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()


def check(spec, flow, unc, f0, n, left, top, h0, w0, dests):
    want = expected(spec, flow, unc, f0, f0 + n, left, top, h0, w0)
    launch(flow, unc, f0, n, left, top, h0, w0, spec, dests)
    for key, dest in dests.items():
        assert same(dest.written(n), want[key].contiguous()), key
        assert dest.rest_untouched(n), key
    return want


FULL = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54, min_disp=0.25)


def test_kernel_odd_crop_pitches_and_frame_range():
    """T = 3, 64 x 64 (h = w = 16), crop 37 x 50 at (13, 7), frames [1, 3), u16 / u16 / u8 at once; pitches 102 / 106 / 53 bytes (wider than the
    row, no multiple of 8); destinations of 4 frames with a gap between frames, written from frame 1 on: frames 0 and 3 stay."""
    flow, unc = engine_state(3, 64, 64, 31)
    spec = OutputSpec(**FULL)
    dests = {"disparity": Dest("u16", 4, 37, 50, pitch_extra=2, first=1, frame_gap=6), "depth": Dest("u16", 4, 37, 50, pitch_extra=6, first=1),
             "uncertainties": Dest("u8", 4, 37, 50, pitch_extra=3, first=1, frame_gap=5)}
    assert [d.pitch for d in dests.values()] == [102, 106, 53] and all(d.pitch % 8 for d in dests.values())
    want = check(spec, flow, unc, 1, 2, 7, 13, 37, 50, dests)
    d16 = want["disparity"].to(torch.int32)
    assert (d16 == 0).any() and (d16 == 65535).any() and ((d16 > 0) & (d16 < 65535)).any() and (want["depth"].to(torch.int32) == 0).any()


def test_kernel_float_formats_uncropped():
    """32 x 64 uncropped (the bottom and right clamps of the bilinear expression are reached): f32 / f32 / f32, then f16 / f16; the f32 planes
    are flow_up[:, :1].abs() and ppms_bilinear(...).abs() themselves."""
    flow, unc = engine_state(3, 32, 64, 32)
    dests = {"disparity": Dest("f32", 3, 32, 64), "depth": Dest("f32", 3, 32, 64), "uncertainties": Dest("f32", 3, 32, 64)}
    check(OutputSpec(disparity="f32", depth="f32", uncertainty="f32", focal_px=721.5377, baseline=0.54, min_disp=0.25), flow, unc, 0, 3, 0, 0, 32, 64, dests)
    assert same(dests["disparity"].written(3), flow[:, :1].abs().cpu())
    assert torch.equal(dests["uncertainties"].written(3), bilinear(unc.view(3, 1, 8, 16), (32, 64), False).abs().cpu())
    z = dests["depth"].written(3)
    assert torch.isposinf(z).any() and torch.isfinite(z).any() and not z.isnan().any()
    dests = {"disparity": Dest("f16", 3, 32, 64), "depth": Dest("f16", 3, 32, 64), "uncertainties": Dest("f32", 3, 32, 64)}
    check(OutputSpec(disparity="f16", depth="f16", uncertainty="f32", focal_px=721.5377, baseline=0.54, min_disp=0.25), flow, unc, 0, 3, 0, 0, 32, 64, dests)


@pytest.mark.parametrize("formats", [("u16", "u16", "u8"), ("f32", "f32", "f32")])
def test_kernel_vector_and_scalar_store_branches(formats):
    """Crop 32 x 64 of 32 x 68.  pad_left = 0, pitch = row: every run starts 16-byte aligned (vector loads and stores).  pad_left = 1 and a pitch
    of row + one element pair: the source rows are unaligned and the destination rows are aligned in some rows only -- both store branches in
    one launch."""
    flow, unc = engine_state(2, 32, 68, 33)
    spec = OutputSpec(disparity=formats[0], depth=formats[1], uncertainty=formats[2], focal_px=721.5377, baseline=0.54, min_disp=0.25)
    dense = {k: Dest(f, 2, 32, 64) for k, f in zip(KEYS, formats)}
    assert all(d.buf.data_ptr() % 16 == 0 and d.pitch % 16 == 0 for d in dense.values())
    check(spec, flow, unc, 0, 2, 0, 0, 32, 64, dense)
    odd = {k: Dest(f, 2, 32, 64, pitch_extra=2 * FMT[f][2]) for k, f in zip(KEYS, formats)}
    assert all(d.pitch % 16 for d in odd.values())
    check(spec, flow, unc, 0, 2, 1, 0, 32, 64, odd)


@pytest.mark.parametrize("only", KEYS)
def test_kernel_skipped_planes(only):
    """One plane alone, the other two NULL: their buffers stay as they were, and the constants of a skipped plane are not looked at."""
    flow, unc = engine_state(2, 32, 64, 34)
    spec = OutputSpec(**FULL)
    want = expected(spec, flow, unc, 0, 2, 3, 2, 27, 59)
    dests = {"disparity": Dest("u16", 2, 27, 59), "depth": Dest("u16", 2, 27, 59), "uncertainties": Dest("u8", 2, 27, 59)}
    if only != "depth":
        spec.fb, spec.depth_scale, spec.min_disp = 0.0, 0.0, float("nan")
    if only != "disparity":
        spec.disp_scale = 0.0
    launch(flow, unc, 0, 2, 3, 2, 27, 59, spec, {only: dests[only]})
    for key, dest in dests.items():
        if key == only:
            assert same(dest.written(2), want[key].contiguous()) and dest.rest_untouched(2)
        else:
            assert dest.untouched(), key


def test_kernel_output_frame_stride_past_2_to_31():
    """Two frames of 8 x 12 whose second lies (1 << 31) + 4097 bytes behind the first in one uint8 allocation (the u8 plane; + 4098 for the
    2-byte disparity): the destination offset is 64-bit arithmetic."""
    flow, unc = engine_state(2, 8, 12, 35)
    spec = OutputSpec(disparity="u16", uncertainty="u8")
    want = expected(spec, flow, unc, 0, 2, 0, 0, 8, 12)
    for key, fmt, stride in (("uncertainties", "u8", (1 << 31) + 4097), ("disparity", "u16", (1 << 31) + 4098)):
        es, frame = FMT[fmt][2], 8 * 12 * FMT[fmt][2]
        buf = torch.empty(stride + frame + 64, dtype=torch.uint8, device=DEV)
        near = [slice(0, frame + 64), slice(stride - 64, stride + frame + 64)]
        for s in near:
            buf[s] = 0x5A
        plane = L.EgressPlane(buf.data_ptr(), stride, 12 * es, FMT[fmt][0], 0)
        planes = {"disparity": NO_PLANE, "depth": NO_PLANE, "uncertainties": NO_PLANE, key: plane}
        out = L.Egress(planes["disparity"], planes["depth"], planes["uncertainties"], spec.disp_scale, 0.0, 0.0, 0.0)
        with torch.cuda.device(DEV):
            L.check(L.load().ppms_disparity_egress(flow.data_ptr(), unc.data_ptr(), 2, 8, 12, 0, 2, 0, 0, 8, 12, ctypes.byref(out), L.stream_ptr()))
            torch.cuda.synchronize()
        got = torch.stack([buf[t * stride:t * stride + frame].cpu().view(FMT[fmt][1]).reshape(1, 8, 12) for t in range(2)])
        assert same(got, want[key].contiguous()), key
        assert (buf[frame:frame + 64] == 0x5A).all() and (buf[stride - 64:stride] == 0x5A).all() and (buf[stride + frame:] == 0x5A).all()
        del buf


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def rand_u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def model():
    """PPMStereo.shipped() with this package's encoders and the procedural weights (as tests/test_gpu_ingest_u8.py builds it)."""
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd.ppmstereo import PPMStereo
    m = PPMStereo.shipped()
    m.load_hot_path_weights(W)
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True)
    m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


QUANT = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54)


def same_results(a, b, keys=("disparity", "uncertainties")):
    return all(same(a[k], b[k]) for k in keys)


def against_default(model, video, n, **kw):
    """The two comparisons every window layout gets: OutputSpec() returns the default call's tensors; u16 / u16 / u8 the reference of them."""
    run = lambda v, **o: model.forward_batch_test({"stereo_video": v}, **kw, **o)
    ref, ref2 = run(video), run(video)
    assert same_results(ref, ref2), "the default path itself is not repeatable: nothing can be said about the egress path"
    out = run(video, output=OutputSpec())
    assert set(out) == {"disparity", "uncertainties"} and tuple(out["disparity"].shape) == (n, 1, 60, 250) and not out["disparity"].is_cuda
    assert out["disparity"].is_pinned() and same_results(out, ref)
    spec = OutputSpec(**QUANT)
    q = run(video, output=spec)
    want = spec.reference(ref["disparity"], ref["uncertainties"])
    assert set(q) == set(KEYS) and [q[k].dtype for k in KEYS] == [torch.uint16, torch.uint16, torch.uint8]
    assert same_results(q, want, KEYS)
    assert (q["disparity"].to(torch.int32) > 0).any() and (q["uncertainties"] > 0).any()
    only = run(video, output=OutputSpec(disparity="f16", uncertainty=None))
    assert set(only) == {"disparity"} and same(only["disparity"], ref["disparity"].to(torch.float16))
    return run, ref


def test_model_single_window(model):
    against_default(model, rand_u8((3, 2, 3, 60, 250), 41), 3, kernel_size=20, iters=4)


def test_model_several_windows_take_the_clip_pipeline(model):
    """Three windows: every kept frame lands in its slice and none is stale; the attention accounting is the default call's."""
    from ppmstereo_amd.ppmstereo import window_plan
    assert len(window_plan(7, 4)) == 3
    run, ref = against_default(model, rand_u8((7, 2, 3, 60, 250), 42), 7, kernel_size=4, iters=2)
    video = rand_u8((7, 2, 3, 60, 250), 42)
    dref = run(video, diagnostics=True)
    dout = run(video, diagnostics=True, output=OutputSpec(disparity="u16", uncertainty="u8"))
    assert dref["attn_redo"] and dout["attn_redo"] == dref["attn_redo"]
    assert same(dout["disparity"], OutputSpec(disparity="u16", uncertainty="u8").reference(ref["disparity"], ref["uncertainties"])["disparity"])


def test_model_forward_directly(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 43).to(DEV), rand_u8((1, 3, 3, 64, 256), 44).to(DEV)
    rd, ru = model.forward(i1, i2, iters=4, test_mode=True)
    spec = OutputSpec(disparity="u16")
    out = model.forward(i1, i2, iters=4, test_mode=True, output=spec, frames=(1, 3))
    torch.cuda.synchronize()
    want = spec.reference(rd[:, 1:3].cpu(), ru[:, 1:3].cpu())
    assert set(out) == {"disparity", "uncertainties"} and tuple(out["disparity"].shape) == (1, 2, 1, 64, 256) and out["disparity"].is_cuda
    assert same_results({k: v.cpu() for k, v in out.items()}, want)
    crop = model.forward(i1, i2, iters=4, test_mode=True, output=spec, crop=(5, 3, 40, 200))
    torch.cuda.synchronize()
    want = spec.reference(rd[..., 3:43, 5:205].cpu(), ru[..., 3:43, 5:205].cpu())
    assert tuple(crop["disparity"].shape) == (1, 3, 1, 40, 200) and same_results({k: v.cpu() for k, v in crop.items()}, want)


def test_model_yuv_video(model):
    from ppmstereo_amd.ppmstereo import YUVFrames, YUVStereoVideo
    views = [YUVFrames(rand_u8((3, 60, 250), 45 + i), rand_u8((3, 30, 125), 47 + i), rand_u8((3, 30, 125), 49 + i)) for i in range(2)]
    spec = OutputSpec(**QUANT)
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4, output=spec)
    out = run(YUVStereoVideo(*views))
    ref = run(torch.stack([views[0].to_rgb_u8(), views[1].to_rgb_u8()], dim=1))
    assert tuple(out["depth"].shape) == (3, 1, 60, 250) and same_results(out, ref, KEYS)


def test_model_refusals(model, monkeypatch):
    v = rand_u8((1, 2, 3, 64, 256), 51).to(DEV)
    with pytest.raises(NotImplementedError):
        model.forward(v, v, iters=2, test_mode=False, output=OutputSpec())
    with pytest.raises(NotImplementedError):
        model.forward(v.expand(2, -1, -1, -1, -1), v.expand(2, -1, -1, -1, -1), iters=2, test_mode=True, output=OutputSpec())
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError):
        model.forward_batch_test({"stereo_video": rand_u8((3, 2, 3, 60, 250), 52)}, kernel_size=20, iters=2, shard_ranks=True, output=OutputSpec())
