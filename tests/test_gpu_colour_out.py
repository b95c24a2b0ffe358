"""GPU: colour out.  video_colour_kernel behind every door against ``colour_bytes`` of the source's left float views; its geometry (a rectangle
that reaches into the replicate padding, unaligned rows, pitches, one column, a frame stride past 2^31); the coloured compact cloud
(ppms_cloud_egress_colour) against ``OutputSpec.reference`` evaluated on the host, with a colour plane a quarter of whose pixels hold the 32 bits of
a signalling NaN; the launches beside the old ones; PPMStereo.forward / forward_batch_test with ``colour=`` and the "xyzrgb" cloud.  Every
comparison is of bytes or of int32 words: there is no tolerance.  Destinations are poisoned first, and what a call must not write is checked for
the poison."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from colour_util import ColourDest, door_source, padded_float, random_colour_plane
from egress_util import (GATES, POISON, RIG_CAL, B, CloudDest, F, Q, bilinear, engine_state, model, model_refuses, rand_u8, same_results)  # noqa: F401  (model: the fixture)
from ingest_util import rotated_map
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec, StereoRectifier, colour_bytes, stereo_source
from test_gpu_block import DEV
from test_gpu_egress_cloud import A_GEOMETRY

pytestmark = pytest.mark.gpu


# ---- 1. kernel A behind every door --------------------------------------------------------------------------------------------------------------
DOORS = [("u8", "rgba8"), ("nv12", "bgra8"), ("yuv422p12", "rgba8"), ("raw12", "bgra8"), ("v210", "rgba8"), ("raw10p", "bgra8")]
DOOR_CASES = [(door, twin, order if not twin else {"rgba8": "bgra8", "bgra8": "rgba8"}[order]) for door, order in DOORS for twin in (False, True)]
DOOR_CASES.append(("p010", False, "bgra8"))


@pytest.mark.parametrize("door,twin,order", DOOR_CASES, ids=[f"{d}{'_remap' if t else ''}-{o}" for d, t, o in DOOR_CASES])
def test_kernel_a_every_door(door, twin, order):
    """N = 3 frames per view, frames [1, 3) of the left one, 37 x 50 (the twins: 40 x 56 raw frames behind maps that turn the views and reach over
    the frame's corners, constant border: fill pixels appear).  The plane lies 16 bytes into a poisoned allocation with 8 bytes between its frames."""
    rectify = None
    if twin:
        rectify = StereoRectifier(rotated_map(37, 50, 40, 56, 0.21, 1.2, "constant", 200), rotated_map(37, 50, 40, 56, -0.17, 1.25, "constant", 200))
    with torch.cuda.device(DEV):
        source = door_source(door, (40, 56) if twin else (37, 50), 700 + 7 * len(door), rectify)
        assert source.size == (37, 50) and source.n == 3 and source._entry.endswith("_remap") == twin
        dest = ColourDest(2, 37, 50, frame_gap=8, lead=16)
        source.colour(dest.plane, 1, 2, 0, 0, 37, 50, order)
        left = source.float_views()[0]
        want = colour_bytes(left[1:3], order)
        dest.check(want)
    assert tuple(left.shape) == (3, 3, 37, 50) and len(want[..., :3].unique()) > 100 and bool((want[..., 3] == 255).all())
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[0], colour_bytes(left[0:1], order)[0])      # the frames differ: frame0 counts
    if twin:                                                    # the constant border's fill: the table's byte of level_fill, in all three channels
        fill = source._colour_table()[rectify.left.level_fill(source.depth)]
        assert bool((want[:, 0, 0, :3] == fill).all()) and bool((want[:, -1, -1, :3] == fill).all())


# ---- 2. kernel A: geometry, on the u8 door ------------------------------------------------------------------------------------------------------
def u8_source(seed=731):
    return door_source("u8", (37, 50), seed)


@pytest.mark.parametrize("rect,dest_kw", [((-7, -13, 64, 64), dict(pitch_extra=0)),                         # reaches into all four paddings
                                          ((0, 0, 37, 50), dict(pitch_extra=0)),                          # rows of 200 bytes: unaligned from row 1 on
                                          ((0, 0, 37, 50), dict(pitch_extra=12, frame_gap=4, lead=4)),    # a pitch of 4 * w0 + 12, nothing aligned
                                          ((49, 36, 3, 1), dict(pitch_extra=4)),                          # w0 = 1, over the bottom right corner
                                          ((-60, 40, 5, 9), dict()), ((3, 5, 30, 43), dict(lead=8))],
                         ids=["into_the_padding", "dense_w50", "pitched", "w0_1", "all_outside", "inside"])
def test_kernel_a_geometry(rect, dest_kw):
    x0, y0, h0, w0 = rect
    with torch.cuda.device(DEV):
        source = u8_source()
        dest = ColourDest(2, h0, w0, **dest_kw)
        source.colour(dest.plane, 1, 2, x0, y0, h0, w0, "bgra8")
        dest.check(colour_bytes(padded_float(source.float_views()[0][1:3], x0, y0, h0, w0), "bgra8"))


def test_kernel_a_frame_stride_past_2_to_31():
    """Two frames of 8 x 12 pixels (1 << 31) + 4100 bytes apart in one allocation: the destination offset is 64-bit arithmetic."""
    stride, frame = (1 << 31) + 4100, 8 * 12 * 4
    with torch.cuda.device(DEV):
        source = u8_source()
        buf = torch.empty(stride + frame + 64, dtype=torch.uint8, device=DEV)
        for s in (slice(0, frame + 64), slice(stride - 64, stride + frame + 64)):
            buf[s] = POISON
        plane = torch.as_strided(buf, (2, 8, 12, 4), (stride, 48, 4, 1))
        source.colour(plane, 1, 2, 20, 10, 8, 12, "rgba8")
        want = colour_bytes(source.float_views()[0][1:3, :, 10:18, 20:32], "rgba8").cpu()
        torch.cuda.synchronize()
        for f in range(2):
            got = buf[f * stride:f * stride + frame + 64].cpu()
            assert torch.equal(got[:frame], want[f].flatten()) and (got[frame:] == POISON).all()
        assert (buf[stride - 64:stride] == POISON).all()
        del buf, plane


# ---- 3. kernel B: the coloured compact cloud ----------------------------------------------------------------------------------------------------
ENTRY = "ppms_cloud_egress_colour"


def colour_spec(order="bgra8", **kw):
    return OutputSpec(colour=order, cloud="f32", cloud_layout="xyzrgb", cloud_index=True, Q=Q, **{**RIG_CAL, **GATES, **kw})


def expected(spec, flow, unc, colour, f0, n, left, top, h0, w0):
    """egress_util.expected with the colour plane: OutputSpec.reference on the host."""
    T, _, H, Wd = flow.shape
    up = bilinear(unc.view(T, 1, H // 4, Wd // 4), (H, Wd), False)
    cut = lambda x: x[f0:f0 + n, :1, top:top + h0, left:left + w0].cpu()
    return spec.reference(cut(flow), cut(up), colour)


def launch_colour(spec, dest, flow, unc, plane_struct, f0, n, left, top, h0, w0):
    T, _, H, Wd = flow.shape
    out = dest.struct(spec, n, h0, w0)
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_cloud_egress_colour(flow.data_ptr(), unc.data_ptr(), T, H, Wd, f0, n, left, top, h0, w0, ctypes.byref(out),
                                                  ctypes.byref(plane_struct), L.stream_ptr()))
        torch.cuda.synchronize()


def on_device(colour, order, **dest_kw):
    """The host colour plane in a (pitched) device allocation -> (its keeper, the ppms_egress_plane)."""
    n, h0, w0, _ = colour.shape
    keep = ColourDest(n, h0, w0, **dest_kw)
    keep.plane.copy_(colour.to(DEV))
    return keep, keep.struct(order)


def check_colour_cloud(spec, flow, unc, geometry, dest, seed, capacity_hit=False, order="bgra8", partial=True, **dest_kw):
    f0, n, left, top, h0, w0 = geometry
    colour = random_colour_plane(n, h0, w0, seed, order)
    want = expected(spec, flow, unc, colour, *geometry)
    counts = want["cloud_counts"].tolist()
    assert not partial or all(0 < c < h0 * w0 for c in counts), counts
    keep, plane = on_device(colour, order, **dest_kw)
    launch_colour(spec, dest, flow, unc, plane, *geometry)
    dest.check(n, want, capacity_hit)
    keep.check(colour)                                          # the plane is read, never written
    return want, colour


def test_kernel_b_frame_spans_two_workgroups_both_gates():
    """test_gpu_egress_cloud's A geometry: frames [1, 3) of T = 3, the 37 x 50 crop of 64 x 64 -- two workgroups per frame, every row ends in a
    2-pixel run, rows of 200 bytes (unaligned from row 1 on).  Records 4 bytes off the allocation's alignment, gaps between the frames."""
    flow, unc = engine_state(3, 64, 64, 71)
    dest = CloudDest("f32", 4, 4, 37 * 50, first=1, gap=40, index_gap=12, lead=4)
    want, colour = check_colour_cloud(colour_spec(), flow, unc, A_GEOMETRY, dest, 811)
    words = colour.view(torch.int32).reshape(2, -1)
    for f in range(2):                                          # the definition once more, read off the plane: word k is the pixel at index k
        fourth = want["cloud"][f].view(torch.int32)[:, 3]
        assert torch.equal(fourth, words[f][want["cloud_index"][f].long()]) and int(((fourth >> 22) & 0x3FF == 0x3FE).sum()) > 20


def test_kernel_b_pitched_colour_plane_and_the_other_order():
    flow, unc = engine_state(3, 64, 64, 72)
    check_colour_cloud(colour_spec("rgba8"), flow, unc, A_GEOMETRY, CloudDest("f32", 4, 4, 37 * 50, first=1), 812, order="rgba8", pitch_extra=12,
                       frame_gap=20, lead=4)


def test_kernel_b_capacity_cuts_inside_the_second_workgroup():
    flow, unc = engine_state(3, 64, 64, 75)
    spec = colour_spec()
    want = expected(spec, flow, unc, random_colour_plane(2, 37, 50, 813), *A_GEOMETRY)
    first_wg = int(want["cloud_index"][0].lt(36 * 50 + 32).sum())       # frame 0's second workgroup has 3 runs: pixel 36 * 50 + 32 onward
    assert int(want["cloud_counts"][0]) - first_wg >= 2
    cut = first_wg + (int(want["cloud_counts"][0]) - first_wg) // 2
    check_colour_cloud(spec, flow, unc, A_GEOMETRY, CloudDest("f32", 4, 4, cut, first=1, gap=24, index_gap=8), 813, capacity_hit=True)


def test_kernel_b_more_workgroups_than_a_workgroup_has_threads():
    """test_gpu_egress_cloud's geometry of that name: T = 1, 516 x 1024 uncropped, 258 workgroups of 256 in the frame -- the reduction that gives the
    last workgroups their base takes more than one block count per thread."""
    assert L.load().ppms_cloud_egress_workspace(1, 516, 1024) == 258
    flow, unc = engine_state(1, 516, 1024, 76)
    check_colour_cloud(colour_spec(), flow, unc, (0, 1, 0, 0, 516, 1024), CloudDest("f32", 4, 1, 516 * 1024), 818)


def test_kernel_b_one_full_workgroup_without_the_uncertainty_gate():
    """32 x 64 uncropped, T = 2: exactly 256 whole, 16-byte aligned runs per frame -- the 16-byte loads of the colour words.  max_uncertainty off:
    nothing reads unc, and NULL is accepted for it."""
    flow, unc = engine_state(2, 32, 64, 72)
    spec = colour_spec(max_uncertainty=None)
    geometry = (0, 2, 0, 0, 32, 64)
    want, colour = check_colour_cloud(spec, flow, unc, geometry, CloudDest("f32", 4, 2, 32 * 64), 814)
    dest = CloudDest("f32", 4, 2, 32 * 64)
    keep, plane = on_device(colour, "bgra8")
    out = dest.struct(spec, 2, 32, 64)
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_cloud_egress_colour(flow.data_ptr(), None, 2, 32, 64, 0, 2, 0, 0, 32, 64, ctypes.byref(out), ctypes.byref(plane), L.stream_ptr()))
        torch.cuda.synchronize()
    dest.check(2, want)


def test_kernel_b_all_invalid_frames_write_nothing():
    flow, unc = engine_state(2, 32, 68, 73)
    want, _ = check_colour_cloud(colour_spec(min_disp=1000.0), flow, unc, (0, 2, 1, 2, 27, 59), CloudDest("f32", 4, 2, 27 * 59, gap=8), 815, partial=False)
    assert want["cloud_counts"].tolist() == [0, 0]


def test_kernel_b_two_runs_give_identical_bytes_and_xyz_are_cloud_egress_bits():
    """X, Y, Z, counts and indices are those of ppms_cloud_egress with "xyzw" on the same state; only the fourth word differs."""
    flow, unc = engine_state(3, 64, 64, 77)
    spec = colour_spec()
    colour = random_colour_plane(2, 37, 50, 816)
    keep, plane = on_device(colour, "bgra8")
    runs = []
    for _ in range(2):
        dest = CloudDest("f32", 4, 4, 37 * 50, first=1, gap=40, index_gap=12, lead=4)
        launch_colour(spec, dest, flow, unc, plane, *A_GEOMETRY)
        runs.append((dest.records.cpu(), dest.index.cpu(), dest.counts.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and not (runs[0][0] == POISON).all()
    old = CloudDest("f32", 4, 4, 37 * 50, first=1, gap=40, index_gap=12, lead=4)
    xyzw = OutputSpec(cloud="f32", cloud_layout="xyzw", cloud_index=True, Q=Q, **RIG_CAL, **GATES)
    T, _, H, Wd = flow.shape
    with torch.cuda.device(DEV):
        out = old.struct(xyzw, 2, 37, 50)
        L.check(L.load().ppms_cloud_egress(flow.data_ptr(), unc.data_ptr(), T, H, Wd, *A_GEOMETRY, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()
    assert torch.equal(old.counts.cpu(), runs[0][2]) and torch.equal(old.index.cpu(), runs[0][1])
    for fr in (1, 2):
        k = int(old.counts[fr])
        assert 0 < k < 37 * 50
        rec = lambda d: d[4 + fr * old.frame_stride:4 + fr * old.frame_stride + 16 * k].view(torch.int32).reshape(k, 4)
        a, b = rec(runs[0][0]), rec(old.records.cpu())
        assert torch.equal(a[:, :3], b[:, :3]) and not torch.equal(a[:, 3], b[:, 3])


# ---- 4. beside the old launches -----------------------------------------------------------------------------------------------------------------
def test_launch_beside_the_planes_leaves_their_bits():
    """``_EgressCall.launch`` with ``colour=`` and "xyzrgb": "disparity", "depth", "uncertainties" and "points" are the bits of the same spec without
    them; the same spec's cloud with cloud_layout="xyzw" is the bits it was; the coloured cloud has its X, Y, Z and the plane's words."""
    from ppmstereo_amd.engine import ScaleEngine
    from ppmstereo_amd.output import _EgressCall
    flow, unc = engine_state(3, 64, 64, 78)
    eng = SimpleNamespace(FLOW_OUT=flow, UNC=unc, T=3, h=16, w=16, shard=None)
    eng.egress = lambda *a: ScaleEngine.egress(eng, *a)
    kw = dict(disparity="u16", depth="u16", uncertainty="u8", points="f32", points_layout="xyzw", Q=Q, cloud="f32", cloud_index=True, **RIG_CAL, **GATES)
    colour = random_colour_plane(2, 37, 50, 817).to(DEV)

    def launch(spec, plane=None):
        call = _EgressCall(spec, A_GEOMETRY[2:], (1, 3))
        call.colour = plane
        return call.launch(eng)
    with torch.cuda.device(DEV):
        plain = launch(OutputSpec(cloud_layout="xyzw", **kw))
        both = launch(OutputSpec(colour="bgra8", cloud_layout="xyzrgb", **kw), colour)
        beside = launch(OutputSpec(colour="bgra8", cloud_layout="xyzw", **kw), colour)
        hidden = launch(OutputSpec(colour="bgra8", colour_plane=False, cloud_layout="xyzrgb", **kw), colour)
        with pytest.raises(RuntimeError):
            launch(OutputSpec(colour="bgra8", cloud_layout="xyzrgb", **kw))
        torch.cuda.synchronize()
    old = ["disparity", "depth", "uncertainties", "points"]
    assert list(plain) == old + ["cloud", "cloud_counts", "cloud_index"] and list(both) == list(beside) == old + ["colour", "cloud", "cloud_counts", "cloud_index"]
    assert list(hidden) == list(plain) and both["colour"] is colour
    words = colour.view(torch.int32).reshape(2, -1)
    for other in (both, beside, hidden):
        assert same_results(other, plain, old + ["cloud_counts"])
    for f, count in enumerate(plain["cloud_counts"].tolist()):          # (rows past a frame's records are never written)
        assert 0 < count < 37 * 50
        assert all(torch.equal(o["cloud_index"][f, :count], plain["cloud_index"][f, :count]) for o in (both, beside, hidden))
        assert torch.equal(beside["cloud"][f, :count].view(torch.int32), plain["cloud"][f, :count].view(torch.int32))
        for coloured in (both, hidden):
            got, was = coloured["cloud"][f, :count].view(torch.int32), plain["cloud"][f, :count].view(torch.int32)
            assert torch.equal(got[:, :3], was[:, :3]) and torch.equal(got[:, 3], words[f][plain["cloud_index"][f, :count].long()])


# ---- 5. the model ---------------------------------------------------------------------------------------------------------------------------------
def specs(ref_u, order="bgra8", **kw):
    """(the coloured spec, the same spec without colour and with the "xyzw" cloud): u16 / u8 planes and a cloud gated at the median of the default
    call's own uncertainty, so that valid and invalid pixels both occur whatever the procedural weights produce."""
    base = dict(disparity="u16", uncertainty="u8", cloud="f32", cloud_index=True, Q=OutputSpec.q_matrix(F, B, 125.0, 30.0),
                max_uncertainty=float(ref_u.abs().float().nanmedian()), **kw)
    return OutputSpec(colour=order, cloud_layout="xyzrgb", **base), OutputSpec(cloud_layout="xyzw", **base)


def coloured_against_plain(out, plain, left, order, colour_key=True):
    """out: the coloured call's host result; plain: the same call without colour; left: the source's left float views of the kept frames (n, 3, h,
    w).  "colour" is colour_bytes of them; a record's fourth word is the colour pixel at its index; everything else is the plain call's bits."""
    n, _, h, w = left.shape
    want = colour_bytes(left, order).cpu()
    assert list(out) == ["disparity", "uncertainties"] + ["colour"] * colour_key + ["cloud", "cloud_counts", "cloud_index"]
    if colour_key:
        assert out["colour"].dtype == torch.uint8 and tuple(out["colour"].shape) == (n, h, w, 4) and torch.equal(out["colour"], want)
    assert same_results(out, plain) and torch.equal(out["cloud_counts"], plain["cloud_counts"])
    words = want.view(torch.int32).reshape(n, -1)
    counts = out["cloud_counts"].tolist()
    assert len(out["cloud"]) == n and all(0 < c < h * w for c in counts), counts
    for f in range(n):
        got, was = out["cloud"][f].contiguous().view(torch.int32), plain["cloud"][f].contiguous().view(torch.int32)
        assert tuple(got.shape) == (counts[f], 4) and torch.equal(out["cloud_index"][f], plain["cloud_index"][f])
        assert torch.equal(got[:, :3], was[:, :3]) and torch.equal(got[:, 3], words[f][out["cloud_index"][f].long()])


def left_views(video, rectify=None):
    """The left float views of a whole host video, made on the device as the model's sources make them."""
    with torch.cuda.device(DEV):
        return stereo_source("colour test", video[0:len(video)].to(DEV), rectify=rectify).float_views()[0]


def batch_case(model, video, order="bgra8", rectify=None, kernel_size=20, iters=2):
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=kernel_size, iters=iters, rectify=rectify, **o)
    ref = run()
    coloured, plain = specs(ref["uncertainties"], order)
    out = run(output=coloured)
    coloured_against_plain(out, run(output=plain), left_views(video, rectify), order)
    return run, out, coloured


def test_model_uint8_video_single_window_and_the_hidden_plane(model):
    video = rand_u8((3, 2, 3, 60, 250), 41)
    run, out, spec = batch_case(model, video)
    assert out["colour"].is_pinned() and torch.equal(out["colour"][..., :3], video[:, 0].permute(0, 2, 3, 1).flip(-1))      # bytes in, the same bytes out (B, G, R)
    hidden = OutputSpec(colour="bgra8", colour_plane=False, cloud_layout="xyzrgb", cloud="f32", cloud_index=True, Q=spec.Q, disparity="u16", uncertainty="u8",
                        max_uncertainty=spec.max_uncertainty)
    got = run(output=hidden)
    assert list(got) == ["disparity", "uncertainties", "cloud", "cloud_counts", "cloud_index"] and same_results(got, out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got["cloud"], out["cloud"]))


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    assert len(window_plan(7, 4)) == 3
    batch_case(model, rand_u8((7, 2, 3, 60, 250), 42), "rgba8", kernel_size=4)


def test_model_nv12_video_with_rectify(model):
    """Raw 70 x 262 NV12 frames of an unrectified rig -> the rectified 60 x 250 colour plane and coloured cloud."""
    from ppmstereo_amd.ppmstereo import YUVFrames, YUVStereoVideo
    from test_gpu_ingest_remap import smooth_rectifier
    r = smooth_rectifier(60, 250, 70, 262, 1, "constant", 200)
    views = [YUVFrames.nv12(rand_u8((3, 70, 262), 91 + i), rand_u8((3, 35, 131, 2), 93 + i)) for i in range(2)]
    batch_case(model, YUVStereoVideo(*views), rectify=r)


def test_model_packed_raw10_video(model):
    from ppmstereo_amd.ppmstereo import PackedRawFrames, PackedRawStereoVideo
    tone = (torch.linspace(0.0, 1.0, 1024) ** (1 / 2.2)) * 255.0
    views = [PackedRawFrames(rand_u8((3, 60, 5 * 63), 95 + i), 250, "grbg", 10, "mipi", black=64, gains=(1.5, 1.0, 1.8), tone=tone) for i in range(2)]
    batch_case(model, PackedRawStereoVideo(*views), "rgba8")


def test_model_float_video_takes_the_torch_path(model):
    g = torch.Generator().manual_seed(97)
    video = torch.rand((3, 2, 3, 60, 250), generator=g) * 255.0
    video[0, 0, :, :4, :4] = torch.tensor([0.5, 1.5, 254.5, 255.0])     # ties
    batch_case(model, video)


def test_model_forward_with_a_crop_off_the_origin(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 43).to(DEV), rand_u8((1, 3, 3, 64, 256), 44).to(DEV)
    _, ru = model.forward(i1, i2, iters=2, test_mode=True)
    coloured, plain = specs(ru.cpu())

    def host(o):
        """forward's device tensors as forward_batch_test hands them over."""
        assert all(v.is_cuda and v.shape[0] == 1 for v in o.values())
        o = {k: v[0].cpu() for k, v in o.items()}
        counts = o["cloud_counts"].tolist()
        o["cloud"], o["cloud_index"] = ([o[k][f, :c] for f, c in enumerate(counts)] for k in ("cloud", "cloud_index"))
        o["cloud_counts"] = o["cloud_counts"].long()
        return o
    kw = dict(iters=2, test_mode=True, crop=(5, 3, 40, 200), frames=(1, 3))
    out = model.forward(i1, i2, output=coloured, **kw)
    assert tuple(out["colour"].shape) == (1, 2, 40, 200, 4) and out["colour"].dtype == torch.uint8
    coloured_against_plain(host(out), host(model.forward(i1, i2, output=plain, **kw)), i1[0, 1:3, :, 3:43, 5:205].float(), "bgra8")


def test_model_refusals(model, monkeypatch):
    model_refuses(model, monkeypatch, OutputSpec(colour="rgba8", cloud="f32", cloud_layout="xyzrgb", Q=Q))
