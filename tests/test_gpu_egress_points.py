"""GPU: the point-cloud back door.  ppms_scene_egress on synthetic engine state (built as tests/test_gpu_egress.py builds it) against
OutputSpec.reference evaluated on the host, and PPMStereo.forward / forward_batch_test with an OutputSpec that asks for points and gates against
the reference applied to the default call's float32 results.  Every comparison is exact (NaN equals NaN at the same place: an invalid point's
payload is not part of the definition)."""
import ctypes

import pytest
import torch

from ppmstereo_amd import _lib as L
from ppmstereo_amd.engine import bilinear
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_block import DEV
from test_gpu_egress import FMT, KEYS, NO_PLANE, Dest, engine_state, expected, launch, model, rand_u8, same, same_results  # noqa: F401  (model: a fixture)

pytestmark = pytest.mark.gpu
ALL = KEYS + ("points",)
F, B = 721.5377, 0.54                                        # fb = 389.6: with d in [0, 400), max_depth = 5 gates d < 78
Q = OutputSpec.q_matrix(F, B, 24.3, 17.6)
GATES = dict(max_uncertainty=0.7, max_depth=5.0)
CAL = dict(focal_px=F, baseline=B, min_disp=0.25)


def launch3d(flow, unc, f0, n, left, top, h0, w0, spec, dests):
    """dests: {key: Dest or None}; the points' Dest is a plane of w0 * C elements per row."""
    T, _, H, Wd = flow.shape
    pl = [dests[k].plane() if dests.get(k) is not None else NO_PLANE for k in ALL]
    rest = spec.scene_struct({})                              # Q, the gates and the component count as the spec hands them over
    out = L.Egress3D(L.Egress(pl[0], pl[1], pl[2], spec.disp_scale, spec.fb, spec.depth_scale, spec.min_disp), pl[3], rest.q, rest.max_uncertainty,
                     rest.max_depth, rest.points_components, 0)
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_scene_egress(flow.data_ptr(), unc.data_ptr(), T, H, Wd, f0, n, left, top, h0, w0, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()


def all_kinds(spec, want, flow, unc, f0, n, left, top, h0, w0):
    """On the reference side: valid pixels, pixels the uncertainty gate takes, pixels the depth gate takes, and NaN disparities all occur."""
    T, _, H, Wd = flow.shape
    cut = lambda x: x[f0:f0 + n, 0, top:top + h0, left:left + w0].abs().cpu()
    d, u = cut(flow), cut(bilinear(unc.view(T, 1, H // 4, Wd // 4), (H, Wd), False))
    if "points" in want:
        ok = ~want["points"][..., 2].float().isnan()
    else:
        ok = want["depth"][:, 0].to(torch.int32) != 0 if want["depth"].dtype == torch.uint16 else ~want["depth"][:, 0].float().isinf()
    vd, vu = d >= spec.min_disp, u <= spec.max_uncertainty
    return bool(ok.any() and (vd & ~vu).any() and (vd & vu & ~ok).any() and d.isnan().any() and (~vd & ~d.isnan()).any() and not (ok & ~(vd & vu)).any())


def check3d(spec, flow, unc, f0, n, left, top, h0, w0, dests):
    want = expected(spec, flow, unc, f0, f0 + n, left, top, h0, w0)
    launch3d(flow, unc, f0, n, left, top, h0, w0, spec, dests)
    for key, dest in dests.items():
        got = dest.written(n)
        assert same(got.reshape(n, h0, w0, -1) if key == "points" else got, want[key].contiguous()), key
        assert dest.rest_untouched(n), key
    assert all_kinds(spec, want, flow, unc, f0, n, left, top, h0, w0)
    return want


def test_kernel_odd_crop_pitches_frame_range_and_every_plane():
    """T = 3, 64 x 64, crop 37 x 50 at (13, 7), frames [1, 3): "xyz" f32 points beside u16 disparity, u16 depth and u8 uncertainty, both gates on.
    The points pitch (604 bytes) is wider than the row's 600 and no multiple of 16: three rows in four start off alignment and are stored element
    by element, as every row's last run (2 pixels) is.  Destinations of 4 frames with a gap between frames, written from frame 1 on."""
    flow, unc = engine_state(3, 64, 64, 61)
    spec = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", points="f32", Q=Q, **CAL, **GATES)
    dests = {"disparity": Dest("u16", 4, 37, 50, pitch_extra=2, first=1, frame_gap=6), "depth": Dest("u16", 4, 37, 50, pitch_extra=6, first=1),
             "uncertainties": Dest("u8", 4, 37, 50, pitch_extra=3, first=1, frame_gap=5), "points": Dest("f32", 4, 37, 50 * 3, pitch_extra=4, first=1, frame_gap=8)}
    assert dests["points"].pitch == 604 and dests["points"].pitch % 16 and dests["points"].frame_stride % 16
    want = check3d(spec, flow, unc, 1, 2, 7, 13, 37, 50, dests)
    # the gates reach the depth plane and leave the other two alone
    plain = expected(OutputSpec(disparity="u16", depth="u16", uncertainty="u8", **CAL), flow, unc, 1, 3, 7, 13, 37, 50)
    assert same(want["disparity"], plain["disparity"]) and same(want["uncertainties"], plain["uncertainties"]) and not same(want["depth"], plain["depth"])


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzw"), ("f16", "xyz"), ("f16", "xyzw")])
def test_kernel_dense_uncropped_formats_and_layouts(fmt, layout):
    """32 x 64 uncropped and dense: every run is whole and 16-byte aligned (the 16-byte stores), and the bilinear expression's clamps at the
    bottom and the right are reached.  w of "xyzw" is the upsampled |uncertainty| in the points' format, for valid and invalid points alike."""
    flow, unc = engine_state(2, 32, 64, 62)
    C = 4 if layout == "xyzw" else 3
    spec = OutputSpec(disparity="f32", uncertainty="f32", points=fmt, points_layout=layout, Q=Q, **CAL, **GATES)
    dests = {"disparity": Dest("f32", 2, 32, 64), "uncertainties": Dest("f32", 2, 32, 64), "points": Dest(fmt, 2, 32, 64 * C)}
    assert dests["points"].buf.data_ptr() % 16 == 0 and dests["points"].pitch % 16 == 0 and dests["points"].frame_stride % 16 == 0
    want = check3d(spec, flow, unc, 0, 2, 0, 0, 32, 64, dests)
    assert tuple(want["points"].shape) == (2, 32, 64, C)
    if C == 4:
        assert same(dests["points"].written(2).reshape(2, 32, 64, 4)[..., 3], dests["uncertainties"].written(2)[:, 0].to(FMT[fmt][1]))


def test_kernel_points_alone():
    """No other plane: the three planes' buffers stay as they were and their constants are not looked at."""
    flow, unc = engine_state(2, 32, 64, 63)
    spec = OutputSpec(points="f32", Q=Q, **CAL, **GATES)
    others = {"disparity": Dest("f32", 2, 27, 59), "depth": Dest("u16", 2, 27, 59), "uncertainties": Dest("u8", 2, 27, 59)}
    dests = {"points": Dest("f32", 2, 27, 59 * 3)}
    want = expected(spec, flow, unc, 0, 2, 3, 2, 27, 59)
    spec.disp_scale, spec.fb, spec.depth_scale = 0.0, 0.0, 0.0
    launch3d(flow, unc, 0, 2, 3, 2, 27, 59, spec, dests)
    assert same(dests["points"].written(2).reshape(2, 27, 59, 3), want["points"].contiguous()) and dests["points"].rest_untouched(2)
    assert all(d.untouched() for d in others.values()) and all_kinds(spec, want, flow, unc, 0, 2, 3, 2, 27, 59)


@pytest.mark.parametrize("depth", ["u16", "f32", "f16"])
def test_kernel_gates_alone(depth):
    """No points: of the three planes the depth plane alone differs from the ungated call's (ppms_disparity_egress), and it is the reference's."""
    flow, unc = engine_state(2, 32, 64, 64)
    kw = dict(disparity="u16", depth=depth, uncertainty="u8", **CAL)
    make = lambda: {"disparity": Dest("u16", 2, 27, 59), "depth": Dest(depth, 2, 27, 59, pitch_extra=FMT[depth][2]), "uncertainties": Dest("u8", 2, 27, 59)}
    gated, plain = make(), make()
    spec = OutputSpec(**kw, **GATES)
    assert spec.scene and "points" not in spec.formats()
    check3d(spec, flow, unc, 0, 2, 3, 2, 27, 59, gated)
    launch(flow, unc, 0, 2, 3, 2, 27, 59, OutputSpec(**kw), plain)
    assert torch.equal(gated["disparity"].buf, plain["disparity"].buf) and torch.equal(gated["uncertainties"].buf, plain["uncertainties"].buf)
    assert not torch.equal(gated["depth"].buf, plain["depth"].buf)
    # a struct with the gates off and no points: the older entry point's bits, plane for plane
    off = make()
    launch3d(flow, unc, 0, 2, 3, 2, 27, 59, OutputSpec(**kw), off)
    assert all(torch.equal(off[k].buf, plain[k].buf) for k in KEYS)


def test_kernel_points_frame_stride_past_2_to_31():
    """Two frames of 8 x 12 "xyz" f32 points (1152 bytes each) whose second lies (1 << 31) + 4100 bytes behind the first in one uint8 allocation:
    the destination offset is 64-bit arithmetic."""
    flow, unc = engine_state(2, 8, 12, 65)
    spec = OutputSpec(points="f32", Q=Q, **CAL, max_uncertainty=0.5, max_depth=3.0)
    want = expected(spec, flow, unc, 0, 2, 0, 0, 8, 12)
    assert all_kinds(spec, want, flow, unc, 0, 2, 0, 0, 8, 12)
    stride, frame = (1 << 31) + 4100, 8 * 12 * 12
    buf = torch.empty(stride + frame + 64, dtype=torch.uint8, device=DEV)
    for s in (slice(0, frame + 64), slice(stride - 64, stride + frame + 64)):
        buf[s] = 0x5A
    rest = spec.scene_struct({})
    out = L.Egress3D(L.Egress(NO_PLANE, NO_PLANE, NO_PLANE, 0.0, 0.0, 0.0, spec.min_disp), L.EgressPlane(buf.data_ptr(), stride, 12 * 12, L.FMT_F32, 0), rest.q,
                     rest.max_uncertainty, rest.max_depth, 3, 0)
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_scene_egress(flow.data_ptr(), unc.data_ptr(), 2, 8, 12, 0, 2, 0, 0, 8, 12, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()
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
    spec = OutputSpec(points="f32", Q=Q, max_uncertainty=0.5)
    v = rand_u8((1, 2, 3, 64, 256), 51).to(DEV)
    with pytest.raises(NotImplementedError):
        model.forward(v, v, iters=2, test_mode=False, output=spec)
    with pytest.raises(NotImplementedError):
        model.forward(v.expand(2, -1, -1, -1, -1), v.expand(2, -1, -1, -1, -1), iters=2, test_mode=True, output=spec)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError):
        model.forward_batch_test({"stereo_video": rand_u8((3, 2, 3, 60, 250), 52)}, kernel_size=20, iters=2, shard_ranks=True, output=spec)
