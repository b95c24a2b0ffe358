"""GPU: the quantised back door.  ppms_disparity_egress on synthetic engine state against OutputSpec.reference applied to ppms_bilinear's
output and the sliced flow_up, and PPMStereo.forward / forward_batch_test with output= against the reference applied to the default call's
float32 results.  Every comparison is exact: the kernel's steps are single fp32 operations rounded to nearest even, the reference's too
(NaN compares equal to NaN at the same place; its payload is not part of the definition)."""
import pytest
import torch

from egress_util import FMT, KEYS, NO_PLANE, Dest, check, engine_state, expected, launch, model, model_refuses, planes_match, planes_struct, rand_u8, same, same_results  # noqa: F401  (model: the fixture)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.engine import bilinear
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_block import DEV

pytestmark = pytest.mark.gpu
ENTRY = "ppms_disparity_egress"


FULL = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54, min_disp=0.25)


def test_kernel_odd_crop_pitches_and_frame_range():
    """T = 3, 64 x 64 (h = w = 16), crop 37 x 50 at (13, 7), frames [1, 3), u16 / u16 / u8 at once; pitches 102 / 106 / 53 bytes (wider than the
    row, no multiple of 8); destinations of 4 frames with a gap between frames, written from frame 1 on: frames 0 and 3 stay."""
    flow, unc = engine_state(3, 64, 64, 31)
    spec = OutputSpec(**FULL)
    dests = {"disparity": Dest("u16", 4, 37, 50, pitch_extra=2, first=1, frame_gap=6), "depth": Dest("u16", 4, 37, 50, pitch_extra=6, first=1),
             "uncertainties": Dest("u8", 4, 37, 50, pitch_extra=3, first=1, frame_gap=5)}
    assert [d.pitch for d in dests.values()] == [102, 106, 53] and all(d.pitch % 8 for d in dests.values())
    want = check(ENTRY, planes_struct(spec, dests), planes_match(dests), spec, flow, unc, 1, 2, 7, 13, 37, 50)
    d16 = want["disparity"].to(torch.int32)
    assert (d16 == 0).any() and (d16 == 65535).any() and ((d16 > 0) & (d16 < 65535)).any() and (want["depth"].to(torch.int32) == 0).any()


def test_kernel_float_formats_uncropped():
    """32 x 64 uncropped (the bottom and right clamps of the bilinear expression are reached): f32 / f32 / f32, then f16 / f16; the f32 planes
    are flow_up[:, :1].abs() and ppms_bilinear(...).abs() themselves."""
    flow, unc = engine_state(3, 32, 64, 32)
    dests = {"disparity": Dest("f32", 3, 32, 64), "depth": Dest("f32", 3, 32, 64), "uncertainties": Dest("f32", 3, 32, 64)}
    spec = OutputSpec(disparity="f32", depth="f32", uncertainty="f32", focal_px=721.5377, baseline=0.54, min_disp=0.25)
    check(ENTRY, planes_struct(spec, dests), planes_match(dests), spec, flow, unc, 0, 3, 0, 0, 32, 64)
    assert same(dests["disparity"].written(3), flow[:, :1].abs().cpu())
    assert torch.equal(dests["uncertainties"].written(3), bilinear(unc.view(3, 1, 8, 16), (32, 64), False).abs().cpu())
    z = dests["depth"].written(3)
    assert torch.isposinf(z).any() and torch.isfinite(z).any() and not z.isnan().any()
    dests = {"disparity": Dest("f16", 3, 32, 64), "depth": Dest("f16", 3, 32, 64), "uncertainties": Dest("f32", 3, 32, 64)}
    spec = OutputSpec(disparity="f16", depth="f16", uncertainty="f32", focal_px=721.5377, baseline=0.54, min_disp=0.25)
    check(ENTRY, planes_struct(spec, dests), planes_match(dests), spec, flow, unc, 0, 3, 0, 0, 32, 64)


@pytest.mark.parametrize("formats", [("u16", "u16", "u8"), ("f32", "f32", "f32")])
def test_kernel_vector_and_scalar_store_branches(formats):
    """Crop 32 x 64 of 32 x 68.  pad_left = 0, pitch = row: every run starts 16-byte aligned (vector loads and stores).  pad_left = 1 and a pitch
    of row + one element pair: the source rows are unaligned and the destination rows are aligned in some rows only -- both store branches in
    one launch."""
    flow, unc = engine_state(2, 32, 68, 33)
    spec = OutputSpec(disparity=formats[0], depth=formats[1], uncertainty=formats[2], focal_px=721.5377, baseline=0.54, min_disp=0.25)
    dense = {k: Dest(f, 2, 32, 64) for k, f in zip(KEYS, formats)}
    assert all(d.buf.data_ptr() % 16 == 0 and d.pitch % 16 == 0 for d in dense.values())
    check(ENTRY, planes_struct(spec, dense), planes_match(dense), spec, flow, unc, 0, 2, 0, 0, 32, 64)
    odd = {k: Dest(f, 2, 32, 64, pitch_extra=2 * FMT[f][2]) for k, f in zip(KEYS, formats)}
    assert all(d.pitch % 16 for d in odd.values())
    check(ENTRY, planes_struct(spec, odd), planes_match(odd), spec, flow, unc, 0, 2, 1, 0, 32, 64)


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
    launch(ENTRY, planes_struct(spec, {only: dests[only]}), flow, unc, 0, 2, 3, 2, 27, 59)
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
        launch(ENTRY, out, flow, unc, 0, 2, 0, 0, 8, 12)
        got = torch.stack([buf[t * stride:t * stride + frame].cpu().view(FMT[fmt][1]).reshape(1, 8, 12) for t in range(2)])
        assert same(got, want[key].contiguous()), key
        assert (buf[frame:frame + 64] == 0x5A).all() and (buf[stride - 64:stride] == 0x5A).all() and (buf[stride + frame:] == 0x5A).all()
        del buf


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
QUANT = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54)


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
    model_refuses(model, monkeypatch, OutputSpec())
