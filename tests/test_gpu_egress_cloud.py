"""GPU: the compact point cloud.  ppms_cloud_egress on synthetic engine state (tests/egress_util.py's) against OutputSpec.reference evaluated
on the host, and PPMStereo.forward / forward_batch_test with an OutputSpec that asks for a cloud against the organised points of the same call
without one.  Every comparison is of bytes: a record of a valid point holds no NaN.  The destinations are filled with a poison byte before the
launch, so that "not written" is checked as well as "written"."""
from types import SimpleNamespace

import pytest
import torch

from egress_util import (ALL, GATES, POISON, RIG_CAL, B, CloudDest, F, Q, all_kinds, check, engine_state, expected, launch, model, model_refuses, rand_u8,  # noqa: F401
                         same_results)                                                                                                  # (model: the fixture)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_block import DEV

pytestmark = pytest.mark.gpu
ENTRY = "ppms_cloud_egress"


def cloud_spec(fmt="f32", layout="xyz", **kw):
    """Cloud and organised points of one format and layout (the points: what ``all_kinds`` and the comparisons read on the reference side)."""
    return OutputSpec(points=fmt, points_layout=layout, cloud=fmt, cloud_layout=layout, cloud_index=True, Q=Q, **{**RIG_CAL, **GATES, **kw})


def check_cloud(spec, flow, unc, f0, n, left, top, h0, w0, dest, kinds=True, capacity_hit=False):
    return check(ENTRY, dest.struct(spec, n, h0, w0), lambda want, *_: dest.check(n, want, capacity_hit), spec, flow, unc, f0, n, left, top, h0, w0, kinds)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
A_GEOMETRY = (1, 2, 7, 13, 37, 50)                              # frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64


def test_kernel_frame_spans_two_workgroups():
    """T = 3, 64 x 64, crop 37 x 50 at (13, 7), frames [1, 3): 7 runs per row, 259 runs per frame -- two workgroups per frame, the second with 3
    runs; every row ends in a 2-pixel run.  f32 "xyz" (12-byte records: a workgroup's first record is 16-byte aligned in one case of four),
    both gates on, an index, gaps between the frames, destinations of 4 frames written from frame 1 on, records 4 bytes off the allocation's
    alignment."""
    assert L.load().ppms_cloud_egress_workspace(2, 37, 50) == 4
    flow, unc = engine_state(3, 64, 64, 71)
    dest = CloudDest("f32", 3, 4, 37 * 50, first=1, gap=40, index_gap=12, lead=4)
    check_cloud(cloud_spec(), flow, unc, *A_GEOMETRY, dest)


@pytest.mark.parametrize("fmt,layout", [("f16", "xyzw"), ("f32", "xyzw"), ("f16", "xyz")])
def test_kernel_one_full_workgroup_formats_and_layouts(fmt, layout):
    """32 x 64 uncropped, T = 2: exactly 256 runs, one full workgroup per frame.  w of "xyzw" is the upsampled |uncertainty| of the valid pixels."""
    assert L.load().ppms_cloud_egress_workspace(2, 32, 64) == 2
    flow, unc = engine_state(2, 32, 64, 72)
    C = 4 if layout == "xyzw" else 3
    check_cloud(cloud_spec(fmt, layout), flow, unc, 0, 2, 0, 0, 32, 64, CloudDest(fmt, C, 2, 32 * 64))


def test_kernel_empty_frames():
    """min_disp above every disparity: counts 0, nothing written."""
    flow, unc = engine_state(2, 32, 68, 73)
    want = check_cloud(cloud_spec(min_disp=1000.0), flow, unc, 0, 2, 1, 2, 27, 59, CloudDest("f32", 3, 2, 27 * 59, gap=8), kinds=False)
    assert want["cloud_counts"].tolist() == [0, 0]


def test_kernel_all_pixels_valid():
    """Gates off, min_disp = 0 and a state without NaN: every pixel is a record, and the cloud is the organised plane reshaped."""
    flow, unc = engine_state(2, 32, 68, 74)
    flow = flow.nan_to_num(nan=3.0)
    spec = cloud_spec("f32", "xyzw", min_disp=0.0, max_uncertainty=None, max_depth=None)
    want = check_cloud(spec, flow, unc, 0, 2, 1, 2, 27, 59, CloudDest("f32", 4, 2, 27 * 59), kinds=False)
    assert want["cloud_counts"].tolist() == [27 * 59] * 2 and not want["points"][..., :3].isnan().any()
    for f in range(2):
        assert torch.equal(want["cloud"][f], want["points"][f].reshape(-1, 4)) and want["cloud_index"][f].tolist() == list(range(27 * 59))


def test_kernel_truncation_at_the_capacity():
    """capacity = 100 below every frame's count: the first 100 records and indices are the reference's first 100, record 100 onward is poison,
    the counts are the full numbers.  The second workgroup of a frame (base >= capacity) writes nothing."""
    flow, unc = engine_state(3, 64, 64, 75)
    want = check_cloud(cloud_spec(), flow, unc, *A_GEOMETRY, CloudDest("f32", 3, 4, 100, first=1, gap=24, index_gap=8), capacity_hit=True)
    assert min(want["cloud_counts"].tolist()) > 100
    # a capacity that cuts inside the records of frame 0's second workgroup (its 3 runs: pixel 36 * 50 + 32 onward)
    first_wg = int(want["cloud_index"][0].lt(36 * 50 + 32).sum())
    assert int(want["cloud_counts"][0]) - first_wg >= 2
    cut = first_wg + (int(want["cloud_counts"][0]) - first_wg) // 2
    check_cloud(cloud_spec("f16", "xyzw"), flow, unc, *A_GEOMETRY, CloudDest("f16", 4, 4, cut, first=1), capacity_hit=True)


def test_kernel_more_workgroups_than_a_workgroup_has_threads():
    """T = 1, 516 x 1024 uncropped: 128 runs per row, 258 workgroups in the frame -- more than a workgroup has threads, so the reduction that
    gives the last workgroups their base takes more than one block count per thread."""
    assert L.load().ppms_cloud_egress_workspace(1, 516, 1024) == 258
    flow, unc = engine_state(1, 516, 1024, 76)
    check_cloud(cloud_spec(), flow, unc, 0, 1, 0, 0, 516, 1024, CloudDest("f32", 3, 1, 516 * 1024))


def test_kernel_frame_stride_past_2_to_31():
    """Two frames of 8 x 12 whose record arrays lie (1 << 31) + 4100 bytes apart in one allocation: the destination offset is 64-bit arithmetic."""
    flow, unc = engine_state(2, 8, 12, 65)
    spec = cloud_spec(max_uncertainty=0.5, max_depth=3.0)
    want = expected(spec, flow, unc, 0, 2, 0, 0, 8, 12)
    assert all_kinds(spec, want, flow, unc, 0, 2, 0, 0, 8, 12)
    stride, frame = (1 << 31) + 4100, 8 * 12 * 12
    buf = torch.empty(stride + frame + 64, dtype=torch.uint8, device=DEV)
    for s in (slice(0, frame + 64), slice(stride - 64, stride + frame + 64)):
        buf[s] = POISON
    small = CloudDest("f32", 3, 2, 8 * 12)                        # its index, counts and workspace; the records go to ``buf``
    out = small.struct(spec, 2, 8, 12)
    out.records, out.frame_stride = buf.data_ptr(), stride
    launch(ENTRY, out, flow, unc, 0, 2, 0, 0, 8, 12)
    assert small.counts.cpu().tolist() == want["cloud_counts"].tolist() and (small.records == POISON).all()
    for f in range(2):
        k = int(want["cloud_counts"][f])
        assert 0 < k < 96
        got = buf[f * stride:f * stride + frame + 64].cpu()
        assert torch.equal(got[:12 * k], want["cloud"][f].contiguous().view(torch.uint8).flatten()) and (got[12 * k:] == POISON).all()
    assert (buf[stride - 64:stride] == POISON).all()
    del buf


def test_kernel_two_runs_give_identical_bytes():
    flow, unc = engine_state(3, 64, 64, 77)
    runs = []
    for _ in range(2):
        dest = CloudDest("f32", 3, 4, 37 * 50, first=1, gap=40, index_gap=12, lead=4)
        launch(ENTRY, dest.struct(cloud_spec(), 2, 37, 50), flow, unc, *A_GEOMETRY)
        runs.append((dest.records.cpu(), dest.index.cpu(), dest.counts.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and not (runs[0][0] == POISON).all()


def test_launch_beside_the_planes_leaves_their_bits():
    """``_EgressCall.launch`` on an engine's state with a spec of three planes, organised points and a cloud: the planes and points are those of the
    same spec without the cloud, bit for bit, and the cloud is the organised plane at its valid pixels."""
    from ppmstereo_amd.engine import ScaleEngine
    from ppmstereo_amd.output import _EgressCall
    flow, unc = engine_state(3, 64, 64, 78)
    eng = SimpleNamespace(FLOW_OUT=flow, UNC=unc, T=3, h=16, w=16, shard=None)
    eng.egress = lambda *a: ScaleEngine.egress(eng, *a)
    kw = dict(disparity="u16", depth="u16", uncertainty="u8", points="f32", points_layout="xyzw", Q=Q, **RIG_CAL, **GATES)
    with torch.cuda.device(DEV):
        plain = _EgressCall(OutputSpec(**kw), A_GEOMETRY[2:], (1, 3)).launch(eng)
        both = _EgressCall(OutputSpec(cloud="f16", cloud_index=True, cloud_capacity=2000, **kw), A_GEOMETRY[2:], (1, 3)).launch(eng)
        torch.cuda.synchronize()
    assert list(plain) == list(ALL) and list(both) == list(ALL) + ["cloud", "cloud_counts", "cloud_index"]
    assert same_results(both, plain, ALL)
    assert tuple(both["cloud"].shape) == (2, 2000, 3) and both["cloud"].dtype == torch.float16 and tuple(both["cloud_index"].shape) == (2, 2000)
    assert both["cloud_counts"].dtype == torch.int32 and tuple(both["cloud_counts"].shape) == (2,)
    pts = plain["points"].cpu()
    for f, count in enumerate(both["cloud_counts"].tolist()):
        valid = ~pts[f, ..., 2].isnan()
        assert 0 < count == int(valid.sum()) <= 2000
        assert torch.equal(both["cloud"][f, :count].cpu(), pts[f][valid][:, :3].to(torch.float16))
        assert torch.equal(both["cloud_index"][f, :count].cpu(), valid.flatten().nonzero().flatten().to(torch.int32))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def gated_specs(ref_d, ref_u, fmt="f32", layout="xyz", **cloud):
    """test_gpu_egress_points.gated_spec's approach: u16 / u16 / u8 planes and points with gates taken from the default call's own results -- the
    medians of its uncertainty and of fb / d --, so that both sides of either gate are populated whatever the procedural weights produce.
    Returns that spec and the same spec with a cloud of the points' format and layout."""
    fb = float(torch.tensor(F) * torch.tensor(B))
    kw = dict(disparity="u16", depth="u16", uncertainty="u8", focal_px=F, baseline=B, max_uncertainty=float(ref_u.abs().float().nanmedian()),
              max_depth=fb / float(ref_d.abs().float().nanmedian()), points=fmt, points_layout=layout, Q=OutputSpec.q_matrix(F, B, 125.0, 30.0))
    return OutputSpec(**kw), OutputSpec(cloud=fmt, cloud_layout=layout, cloud_index=True, **kw, **cloud)


def cloud_against_points(out, organised, n, h0, w0, capacity=None, pinned=True):
    """``out``: the call with a cloud (host tensors); organised: the same call without one.  The planes and organised points are the same bits; the
    cloud of every frame is the organised points at their valid pixels, cut at the capacity; the counts are the full numbers."""
    assert list(organised) == list(ALL) and list(out) == list(ALL) + ["cloud", "cloud_counts", "cloud_index"] and same_results(out, organised, ALL)
    pts = organised["points"].reshape(n, h0, w0, -1)
    valid = ~pts[..., 2].float().isnan()
    counts = valid.flatten(1).sum(1)
    assert valid.any() and (~valid).any()
    assert out["cloud_counts"].dtype == torch.int64 and out["cloud_counts"].reshape(-1).tolist() == counts.tolist()
    cloud, index = out["cloud"], out["cloud_index"]
    assert len(cloud) == len(index) == n
    for f in range(n):
        k = int(counts[f]) if capacity is None else min(int(counts[f]), capacity)
        assert tuple(cloud[f].shape) == (k, pts.shape[-1]) and tuple(index[f].shape) == (k,)          # no row past the records exists
        assert cloud[f].dtype == pts.dtype and index[f].dtype == torch.int32 and not cloud[f].is_cuda
        assert not pinned or k == 0 or (cloud[f].is_pinned() and index[f].is_pinned())
        assert torch.equal(cloud[f].contiguous().view(torch.uint8), pts[f][valid[f]][:k].contiguous().view(torch.uint8))
        assert torch.equal(index[f], valid[f].flatten().nonzero().flatten()[:k].to(torch.int32))
    return counts


def test_model_single_window(model):
    video = rand_u8((3, 2, 3, 60, 250), 41)
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=4, **o)
    ref = run()
    plain, spec = gated_specs(ref["disparity"], ref["uncertainties"])
    out = run(output=spec)
    counts = cloud_against_points(out, run(output=plain), 3, 60, 250)
    # one pinned (N, capacity, C) allocation: the frames' views lie capacity records apart
    assert out["cloud"][1].data_ptr() - out["cloud"][0].data_ptr() == 60 * 250 * 12 and out["cloud_index"][2].data_ptr() - out["cloud_index"][1].data_ptr() == 60 * 250 * 4
    # a capacity below the counts: the views end there, the counts do not
    cap = int(counts.min()) // 2
    plain, spec = gated_specs(ref["disparity"], ref["uncertainties"], "f16", "xyzw", cloud_capacity=cap)
    cloud_against_points(run(output=spec), run(output=plain), 3, 60, 250, capacity=cap)


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    assert len(window_plan(7, 4)) == 3
    video = rand_u8((7, 2, 3, 60, 250), 42)
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=4, iters=2, **o)
    ref = run()
    plain, spec = gated_specs(ref["disparity"], ref["uncertainties"], "f16", "xyzw")
    cloud_against_points(run(output=spec), run(output=plain), 7, 60, 250)


def test_model_forward_directly(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 43).to(DEV), rand_u8((1, 3, 3, 64, 256), 44).to(DEV)
    rd, ru = (x.cpu() for x in model.forward(i1, i2, iters=4, test_mode=True))
    plain, spec = gated_specs(rd, ru, "f32", "xyzw")

    def host(o):
        """forward's device tensors as forward_batch_test hands them over: the frames' records that exist, the counts as int64."""
        o = {k: v.cpu() for k, v in o.items()}
        if "cloud" in o:
            assert tuple(o["cloud"].shape[:2]) == tuple(o["cloud_counts"].shape) == tuple(o["cloud_index"].shape[:2]) and o["cloud_counts"].dtype == torch.int32
            counts = o["cloud_counts"][0].tolist()
            o["cloud"], o["cloud_index"] = ([o[k][0, f, :c] for f, c in enumerate(counts)] for k in ("cloud", "cloud_index"))
            o["cloud_counts"] = o["cloud_counts"][0].long()
        return o

    out = model.forward(i1, i2, iters=4, test_mode=True, output=spec, frames=(1, 3))
    assert out["cloud"].is_cuda and tuple(out["cloud"].shape) == (1, 2, 64 * 256, 4) and tuple(out["cloud_index"].shape) == (1, 2, 64 * 256)
    cloud_against_points(host(out), host(model.forward(i1, i2, iters=4, test_mode=True, output=plain, frames=(1, 3))), 2, 64, 256, pinned=False)
    # a crop: x, y and the pixel index count from the crop's corner, the image the caller fed in
    crop = host(model.forward(i1, i2, iters=4, test_mode=True, output=spec, crop=(5, 3, 40, 200)))
    cloud_against_points(crop, host(model.forward(i1, i2, iters=4, test_mode=True, output=plain, crop=(5, 3, 40, 200))), 3, 40, 200, pinned=False)


def test_model_rectified_uint8_video(model):
    """rectify= in front, the cloud behind: raw 70 x 262 bytes in, the valid points of a 60 x 250 cloud out."""
    from test_gpu_ingest_remap import raw_video, smooth_rectifier
    r = smooth_rectifier(60, 250, 70, 262, 1)
    _, rgb = raw_video(3, 70, 262, 91)
    run = lambda **o: model.forward_batch_test({"stereo_video": rgb}, kernel_size=20, iters=4, rectify=r, **o)
    ref = run()
    plain, spec = gated_specs(ref["disparity"], ref["uncertainties"])
    cloud_against_points(run(output=spec), run(output=plain), 3, 60, 250)


def test_model_refusals(model, monkeypatch):
    model_refuses(model, monkeypatch, OutputSpec(cloud="f32", Q=Q, max_uncertainty=0.5))
