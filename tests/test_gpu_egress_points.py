"""GPU: the point-cloud back door.  ppms_scene_egress on synthetic engine state (tests/egress_util.py's) against
OutputSpec.reference evaluated on the host, and PPMStereo.forward / forward_batch_test with an OutputSpec that asks for points and gates against
the reference applied to the default call's float32 results.  Every comparison is exact (NaN equals NaN at the same place: an invalid point's
payload is not part of the definition)."""
import pytest
import torch

from egress_util import (ALL, FMT, GATES, KEYS, NO_PLANE, RIG_CAL, B, Dest, F, Q, all_kinds, check, engine_state, expected, launch, model, model_refuses, planes_match,  # noqa: F401
                         planes_struct, rand_u8, same, same_results)                                                                                # (model: the fixture)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_block import DEV

pytestmark = pytest.mark.gpu
ENTRY = "ppms_scene_egress"


def test_kernel_odd_crop_pitches_frame_range_and_every_plane():
    """T = 3, 64 x 64, crop 37 x 50 at (13, 7), frames [1, 3): "xyz" f32 points beside u16 disparity, u16 depth and u8 uncertainty, both gates on.
    The points pitch (604 bytes) is wider than the row's 600 and no multiple of 16: three rows in four start off alignment and are stored element
    by element, as every row's last run (2 pixels) is.  Destinations of 4 frames with a gap between frames, written from frame 1 on."""
    flow, unc = engine_state(3, 64, 64, 61)
    spec = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", points="f32", Q=Q, **RIG_CAL, **GATES)
    dests = {"disparity": Dest("u16", 4, 37, 50, pitch_extra=2, first=1, frame_gap=6), "depth": Dest("u16", 4, 37, 50, pitch_extra=6, first=1),
             "uncertainties": Dest("u8", 4, 37, 50, pitch_extra=3, first=1, frame_gap=5), "points": Dest("f32", 4, 37, 50 * 3, pitch_extra=4, first=1, frame_gap=8)}
    assert dests["points"].pitch == 604 and dests["points"].pitch % 16 and dests["points"].frame_stride % 16
    want = check(ENTRY, planes_struct(spec, dests, True), planes_match(dests), spec, flow, unc, 1, 2, 7, 13, 37, 50, kinds=True)
    # the gates reach the depth plane and leave the other two alone
    plain = expected(OutputSpec(disparity="u16", depth="u16", uncertainty="u8", **RIG_CAL), flow, unc, 1, 3, 7, 13, 37, 50)
    assert same(want["disparity"], plain["disparity"]) and same(want["uncertainties"], plain["uncertainties"]) and not same(want["depth"], plain["depth"])


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzw"), ("f16", "xyz"), ("f16", "xyzw")])
def test_kernel_dense_uncropped_formats_and_layouts(fmt, layout):
    """32 x 64 uncropped and dense: every run is whole and 16-byte aligned (the 16-byte stores), and the bilinear expression's clamps at the
    bottom and the right are reached.  w of "xyzw" is the upsampled |uncertainty| in the points' format, for valid and invalid points alike."""
    flow, unc = engine_state(2, 32, 64, 62)
    C = 4 if layout == "xyzw" else 3
    spec = OutputSpec(disparity="f32", uncertainty="f32", points=fmt, points_layout=layout, Q=Q, **RIG_CAL, **GATES)
    dests = {"disparity": Dest("f32", 2, 32, 64), "uncertainties": Dest("f32", 2, 32, 64), "points": Dest(fmt, 2, 32, 64 * C)}
    assert dests["points"].buf.data_ptr() % 16 == 0 and dests["points"].pitch % 16 == 0 and dests["points"].frame_stride % 16 == 0
    want = check(ENTRY, planes_struct(spec, dests, True), planes_match(dests), spec, flow, unc, 0, 2, 0, 0, 32, 64, kinds=True)
    assert tuple(want["points"].shape) == (2, 32, 64, C)
    if C == 4:
        assert same(dests["points"].written(2).reshape(2, 32, 64, 4)[..., 3], dests["uncertainties"].written(2)[:, 0].to(FMT[fmt][1]))


def test_kernel_points_alone():
    """No other plane: the three planes' buffers stay as they were and their constants are not looked at."""
    flow, unc = engine_state(2, 32, 64, 63)
    spec = OutputSpec(points="f32", Q=Q, **RIG_CAL, **GATES)
    others = {"disparity": Dest("f32", 2, 27, 59), "depth": Dest("u16", 2, 27, 59), "uncertainties": Dest("u8", 2, 27, 59)}
    dests = {"points": Dest("f32", 2, 27, 59 * 3)}
    want = expected(spec, flow, unc, 0, 2, 3, 2, 27, 59)
    spec.disp_scale, spec.fb, spec.depth_scale = 0.0, 0.0, 0.0
    launch(ENTRY, planes_struct(spec, dests, True), flow, unc, 0, 2, 3, 2, 27, 59)
    assert same(dests["points"].written(2).reshape(2, 27, 59, 3), want["points"].contiguous()) and dests["points"].rest_untouched(2)
    assert all(d.untouched() for d in others.values()) and all_kinds(spec, want, flow, unc, 0, 2, 3, 2, 27, 59)


@pytest.mark.parametrize("depth", ["u16", "f32", "f16"])
def test_kernel_gates_alone(depth):
    """No points: of the three planes the depth plane alone differs from the ungated call's (ppms_disparity_egress), and it is the reference's."""
    flow, unc = engine_state(2, 32, 64, 64)
    kw = dict(disparity="u16", depth=depth, uncertainty="u8", **RIG_CAL)
    make = lambda: {"disparity": Dest("u16", 2, 27, 59), "depth": Dest(depth, 2, 27, 59, pitch_extra=FMT[depth][2]), "uncertainties": Dest("u8", 2, 27, 59)}
    gated, plain = make(), make()
    spec = OutputSpec(**kw, **GATES)
    assert spec.scene and "points" not in spec.formats()
    check(ENTRY, planes_struct(spec, gated, True), planes_match(gated), spec, flow, unc, 0, 2, 3, 2, 27, 59, kinds=True)
    launch("ppms_disparity_egress", planes_struct(OutputSpec(**kw), plain), flow, unc, 0, 2, 3, 2, 27, 59)
    assert torch.equal(gated["disparity"].buf, plain["disparity"].buf) and torch.equal(gated["uncertainties"].buf, plain["uncertainties"].buf)
    assert not torch.equal(gated["depth"].buf, plain["depth"].buf)
    # a struct with the gates off and no points: the older entry point's bits, plane for plane
    off = make()
    launch(ENTRY, planes_struct(OutputSpec(**kw), off, True), flow, unc, 0, 2, 3, 2, 27, 59)
    assert all(torch.equal(off[k].buf, plain[k].buf) for k in KEYS)


def test_kernel_points_frame_stride_past_2_to_31():
    """Two frames of 8 x 12 "xyz" f32 points (1152 bytes each) whose second lies (1 << 31) + 4100 bytes behind the first in one uint8 allocation:
    the destination offset is 64-bit arithmetic."""
    flow, unc = engine_state(2, 8, 12, 65)
    spec = OutputSpec(points="f32", Q=Q, **RIG_CAL, max_uncertainty=0.5, max_depth=3.0)
    want = expected(spec, flow, unc, 0, 2, 0, 0, 8, 12)
    assert all_kinds(spec, want, flow, unc, 0, 2, 0, 0, 8, 12)
    stride, frame = (1 << 31) + 4100, 8 * 12 * 12
    buf = torch.empty(stride + frame + 64, dtype=torch.uint8, device=DEV)
    for s in (slice(0, frame + 64), slice(stride - 64, stride + frame + 64)):
        buf[s] = 0x5A
    rest = spec.scene_struct({})
    out = L.Egress3D(L.Egress(NO_PLANE, NO_PLANE, NO_PLANE, 0.0, 0.0, 0.0, spec.min_disp), L.EgressPlane(buf.data_ptr(), stride, 12 * 12, L.FMT_F32, 0), rest.q,
                     rest.max_uncertainty, rest.max_depth, 3, 0)
    launch(ENTRY, out, flow, unc, 0, 2, 0, 0, 8, 12)
    got = torch.stack([buf[t * stride:t * stride + frame].cpu().view(torch.float32).reshape(8, 12, 3) for t in range(2)])
    assert same(got, want["points"].contiguous())
    assert (buf[frame:frame + 64] == 0x5A).all() and (buf[stride - 64:stride] == 0x5A).all() and (buf[stride + frame:] == 0x5A).all()
    del buf


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def gated_spec(ref_d, ref_u, points="f32", layout="xyz", **kw):
    """u16 / u16 / u8 planes and points, with gates taken from the default call's own results -- the medians of its uncertainty and of fb / d -- so
    that both sides of either gate are populated whatever the procedural weights produce.  Returns the spec and the same spec without points."""
    fb = float(torch.tensor(F) * torch.tensor(B))
    gates = dict(max_uncertainty=float(ref_u.abs().float().nanmedian()), max_depth=fb / float(ref_d.abs().float().nanmedian()))
    base = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=F, baseline=B, **gates, **kw)
    return OutputSpec(points=points, points_layout=layout, Q=OutputSpec.q_matrix(F, B, 125.0, 30.0), **base), OutputSpec(**base)


def points_against_default(spec, plain, out, out_plain, ref_d, ref_u, shape):
    """``out``: the call with ``spec``; out_plain: with the same spec without points; ref_d, ref_u: the default call's float32 results (on the host)."""
    want = spec.reference(ref_d, ref_u)
    assert list(out) == list(ALL) and tuple(out["points"].shape) == shape and out["points"].dtype == want["points"].dtype
    assert same_results(out, want, ALL) and same_results(out, out_plain, KEYS) and list(out_plain) == list(KEYS)
    valid = ~want["points"][..., 2].float().isnan()
    assert valid.any() and (~valid).any() and (out["depth"].to(torch.int32) == 0).any() and (out["depth"].to(torch.int32) > 0).any()


def test_model_single_window(model):
    video = rand_u8((3, 2, 3, 60, 250), 41)
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=4, **o)
    ref = run()
    spec, plain = gated_spec(ref["disparity"], ref["uncertainties"])
    out = run(output=spec)
    assert out["points"].is_pinned() and not out["points"].is_cuda
    points_against_default(spec, plain, out, run(output=plain), ref["disparity"], ref["uncertainties"], (3, 60, 250, 3))


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    assert len(window_plan(7, 4)) == 3
    video = rand_u8((7, 2, 3, 60, 250), 42)
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=4, iters=2, **o)
    ref = run()
    spec, plain = gated_spec(ref["disparity"], ref["uncertainties"], "f16", "xyzw")
    points_against_default(spec, plain, run(output=spec), run(output=plain), ref["disparity"], ref["uncertainties"], (7, 60, 250, 4))


def test_model_forward_directly(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 43).to(DEV), rand_u8((1, 3, 3, 64, 256), 44).to(DEV)
    rd, ru = (x.cpu() for x in model.forward(i1, i2, iters=4, test_mode=True))
    spec, plain = gated_spec(rd, ru, "f32", "xyzw")
    host = lambda o: {k: v.cpu() for k, v in o.items()}
    out = model.forward(i1, i2, iters=4, test_mode=True, output=spec, frames=(1, 3))
    assert out["points"].is_cuda
    points_against_default(spec, plain, host(out), host(model.forward(i1, i2, iters=4, test_mode=True, output=plain, frames=(1, 3))), rd[:, 1:3], ru[:, 1:3],
                           (1, 2, 64, 256, 4))
    # a crop: x and y count from the crop's corner, the image the caller fed in
    crop = host(model.forward(i1, i2, iters=4, test_mode=True, output=spec, crop=(5, 3, 40, 200)))
    points_against_default(spec, plain, crop, host(model.forward(i1, i2, iters=4, test_mode=True, output=plain, crop=(5, 3, 40, 200))),
                           rd[..., 3:43, 5:205], ru[..., 3:43, 5:205], (1, 3, 40, 200, 4))


def test_model_rectified_uint8_video(model):
    """rectify= in front, points behind: raw 70 x 262 bytes in, a 60 x 250 cloud out, nothing but this package between them."""
    from test_gpu_ingest_remap import raw_video, smooth_rectifier
    r = smooth_rectifier(60, 250, 70, 262, 1)
    _, rgb = raw_video(3, 70, 262, 91)
    run = lambda **o: model.forward_batch_test({"stereo_video": rgb}, kernel_size=20, iters=4, rectify=r, **o)
    ref = run()
    spec, plain = gated_spec(ref["disparity"], ref["uncertainties"])
    points_against_default(spec, plain, run(output=spec), run(output=plain), ref["disparity"], ref["uncertainties"], (3, 60, 250, 3))


def test_model_refusals(model, monkeypatch):
    model_refuses(model, monkeypatch, OutputSpec(points="f32", Q=Q, max_uncertainty=0.5))
