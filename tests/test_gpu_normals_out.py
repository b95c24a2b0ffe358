"""GPU: surface normals out.  ppms_normals_egress (the LDS-tiled stencil kernel) and ppms_cloud_egress_normals (the oriented compact cloud) against
``OutputSpec.reference`` evaluated on the host, on a surface whose pixels cover every stencil kind; the crop's independence of everything outside it;
shapes at every tile seam; the launches beside the old ones; PPMStereo.forward / forward_batch_test with ``normals=`` and the "xyzrgbn" cloud.
Every comparison is of bits (NaN equals NaN in a plane; a record holds none): there is no tolerance.  Destinations are filled with a pattern or a
poison byte first, so that "not written" is checked as well as "written"."""
import ctypes

import pytest
import torch

from colour_util import ColourDest, random_colour_plane
from egress_util import COUNT_POISON, DEV, CloudDest, Dest, F, B, model, model_refuses, rand_u8, same, same_results  # noqa: F401  (model: the fixture)
from normals_util import (A_CROP, N_GATES, N_RIG, Q_REVERSED, TILE_H, TILE_W, every_kind, expected, launch_cloud_normals, launch_normals, stencil_kinds,
                          surface_state, upsampled, crop)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec, colour_bytes, stereo_source

pytestmark = pytest.mark.gpu
Q = N_RIG["Q"]


def state(T=3, H=64, W=64, seed=5):
    flow, unc = surface_state(T, H, W, seed)
    return flow.to(DEV), unc.to(DEV)


class NormalsDest(Dest):
    """egress_util.Dest for a plane of 3 elements per pixel that starts ``lead`` bytes into its allocation."""

    def __init__(self, fmt, frames, h0, w0, lead=0, **kw):
        super().__init__(fmt, frames, h0, w0 * 3, **kw)
        self.lead = lead
        self.pattern = (torch.arange(lead + frames * self.frame_stride, device=DEV) % 251 + 1).to(torch.uint8)
        self.buf = self.pattern.clone()

    def plane(self):
        p = super().plane()
        p.ptr += self.lead
        return p

    def region(self, t, n):
        return torch.as_strided(t, (n, self.h0, self.w0 * self.es), (self.frame_stride, self.pitch, 1), self.lead + self.first * self.frame_stride)

    def normals(self, n):
        return self.written(n).reshape(n, self.h0, self.w0 // 3, 3)


def check_plane(spec, flow, unc, geometry, dest, kinds=False):
    """The reference on the host, the launch, the plane's rows bit for bit and the pattern everywhere else."""
    n, h0, w0 = geometry[1], *geometry[4:]
    want = expected(spec, flow, unc, *geometry)["normals"]
    launch_normals(spec, dest.plane(), flow, unc, *geometry)
    got = dest.normals(n)
    assert same(got, want), f"{int(((got != want) & ~(got.isnan() & want.isnan())).any(-1).sum())} of {n * h0 * w0} normals differ"
    assert dest.rest_untouched(n)
    if kinds:                                                   # condition of the test: the 15 stencil kinds occur on the reference side
        T, _, H, W = flow.shape
        table, _ = stencil_kinds(spec, crop(flow, *geometry).cpu(), crop(upsampled(unc, H, W), *geometry).cpu())
        assert every_kind(table), table.tolist()
    return want


# ---- 1. ppms_normals_egress: frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64 -- one tile per frame, every row ends in a 2-pixel run ------
CASES = [("f32", {}, 0.05, Q, True), ("f32", N_GATES, 0.05, Q, False), ("f16", N_GATES, 0.05, Q, False), ("f16", {}, 0.5, Q, False),
         ("f32", dict(max_depth=12.0), None, Q, False), ("f32", dict(max_depth=12.0), 0.05, Q, True), ("f32", dict(max_uncertainty=0.7), 0.5, Q, False),
         ("f16", dict(max_uncertainty=0.7), None, Q, False), ("f32", {}, 0.05, Q_REVERSED, False), ("f16", {}, None, Q_REVERSED, False)]


@pytest.mark.parametrize("fmt,gates,jump,q,kinds", CASES, ids=[f"{f}-{'+'.join(g) or 'no_gate'}-jump_{j}-{'Q' if q is Q else 'reversed'}" for f, g, j, q, _ in CASES])
def test_normals_plane(fmt, gates, jump, q, kinds):
    """A pitch wider than the row, a gap between the frames, written from frame ``first`` = 1 of a destination of 4."""
    flow, unc = state()
    spec = OutputSpec(normals=fmt, normal_max_jump=jump, min_disp=0.25, Q=q, **gates)
    es = 4 if fmt == "f32" else 2
    want = check_plane(spec, flow, unc, A_CROP, NormalsDest(fmt, 4, 37, 50, pitch_extra=3 * es, first=1, frame_gap=5 * es), kinds)
    valid = ~want[..., 0].isnan()
    assert 500 < int(valid.sum()) < 3700 and not torch.equal(want[0], want[1])            # normals and holes both occur; the frames differ


def test_normals_plane_two_launches_give_identical_bytes():
    flow, unc = state()
    spec = OutputSpec(normals="f32", **N_RIG, **N_GATES)
    runs = []
    for _ in range(2):
        dest = NormalsDest("f32", 2, 37, 50, pitch_extra=8)
        launch_normals(spec, dest.plane(), flow, unc, *A_CROP)
        runs.append(dest.buf.cpu())
    assert torch.equal(*runs)


# ---- 2. crop independence ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), 3.0e38, -1.0e30, 0.0], ids=["nan", "huge", "huge_negative", "zero"])
def test_nothing_outside_the_crop_is_read(fill):
    """Every flow_up value outside the crop and the frame range, all of channel 1, and every unc sample no pixel of the crop taps, overwritten: the
    same bytes.  (The padded frame has values next to the crop's border; a neighbour there does not exist.)"""
    flow, unc = state()
    f0, n, left, top, h0, w0 = A_CROP
    spec = OutputSpec(normals="f32", **N_RIG, **N_GATES)
    clean = NormalsDest("f32", 2, h0, w0)
    want = check_plane(spec, flow, unc, A_CROP, clean)
    other = torch.full_like(flow, fill)
    other[f0:f0 + n, 0, top:top + h0, left:left + w0] = flow[f0:f0 + n, 0, top:top + h0, left:left + w0]
    taps = lambda s0, size, lim: range(int(max(0.25 * (s0 + 0.5) - 0.5, 0.0)), min(int(max(0.25 * (s0 + size - 0.5) - 0.5, 0.0)) + 1, lim - 1) + 1)
    rows, cols = taps(top, h0, 16), taps(left, w0, 16)
    other_unc = torch.full_like(unc, fill)
    other_unc[f0:f0 + n, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = unc[f0:f0 + n, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    assert int((other != flow).sum()) > 3 * 64 * 64 and int((other_unc != unc).sum()) > 200
    dest = NormalsDest("f32", 2, h0, w0)
    launch_normals(spec, dest.plane(), other, other_unc, *A_CROP)
    assert same(dest.normals(n), want) and torch.equal(dest.buf, clean.buf)


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------------------
# (T, H, W of the state; (f0, n, left, top, h0, w0); the format; the destination)
SHAPES = {
    "w0_8": ((3, 64, 64), (1, 2, 7, 13, 37, 8), "f32", dict(pitch_extra=4)),                   # one whole run per row
    "w0_9": ((3, 64, 64), (1, 2, 7, 13, 37, 9), "f16", dict(pitch_extra=2)),                   # a whole run and a 1-pixel run
    "w0_1": ((3, 64, 64), (1, 2, 30, 13, 37, 1), "f32", dict()),                               # no horizontal neighbour: every normal is NaN
    "h0_1": ((3, 64, 64), (0, 3, 5, 20, 1, 50), "f32", dict(frame_gap=12)),                    # no vertical neighbour: every normal is NaN
    "h0_2": ((3, 64, 64), (0, 3, 5, 20, 2, 50), "f16", dict(frame_gap=2)),                     # one-sided vertical tangents only
    "h0_3": ((3, 64, 64), (0, 3, 5, 20, 3, 50), "f32", dict(pitch_extra=4)),
    "at_0_0": ((3, 64, 64), (0, 2, 0, 0, 37, 50), "f32", dict()),
    "ends_at_H_W": ((3, 64, 64), (1, 2, 14, 27, 37, 50), "f16", dict()),
    "whole_frame_aligned_rows": ((3, 64, 64), (0, 3, 0, 0, 64, 64), "f32", dict()),           # 4 tiles down; every run whole, every store 16 bytes
    "whole_frame_aligned_rows_f16": ((2, 32, 64), (0, 2, 0, 0, 32, 64), "f16", dict()),
    # the tile is TILE_H x TILE_W = 16 x 128: 37 x 150 is 3 x 2 tiles, 2 tiles + 5 rows down and 1 tile + 22 columns across -- every seam and rim side occurs
    "larger_than_the_tile": ((2, 40, 160), (0, 2, 5, 2, 37, 150), "f32", dict(pitch_extra=8)),
    "larger_than_the_tile_f16_whole": ((2, 40, 160), (0, 2, 0, 0, 40, 160), "f16", dict()),
    "unaligned_pointer": ((3, 64, 64), (1, 2, 7, 13, 37, 50), "f32", dict(lead=4)),            # one element off the allocation's alignment
    "unaligned_pointer_f16": ((3, 64, 64), (0, 3, 0, 0, 64, 64), "f16", dict(lead=2)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_normals_plane_shapes(name):
    assert (TILE_H, TILE_W) == (16, 128)
    (T, H, W), geometry, fmt, dest_kw = SHAPES[name]
    flow, unc = state(T, H, W, seed=len(name))
    n, h0, w0 = geometry[1], *geometry[4:]
    want = check_plane(OutputSpec(normals=fmt, **N_RIG, max_depth=12.0), flow, unc, geometry, NormalsDest(fmt, n, h0, w0, **dest_kw))
    valid = int((~want[..., 0].isnan()).sum())
    assert valid == 0 if min(h0, w0) == 1 else 0 < valid < n * h0 * w0


# ---- 4. ppms_cloud_egress_normals ----------------------------------------------------------------------------------------------------------------------
class OrientedDest(CloudDest):
    """egress_util.CloudDest with the oriented cloud's workspace (its workgroups are its own)."""

    def struct(self, spec, n, h0, w0):
        st = super().struct(spec, n, h0, w0)
        self.workspace = torch.full((L.load().ppms_cloud_egress_normals_workspace(n, h0, w0),), COUNT_POISON, dtype=torch.int32, device=DEV)
        st.block_counts, st.block_counts_len = self.workspace.data_ptr(), self.workspace.numel()
        return st


def oriented_spec(fmt="f32", layout="xyzn", **kw):
    colour = dict(colour="bgra8") if layout == "xyzrgbn" else {}
    return OutputSpec(normals=fmt, cloud=fmt, cloud_layout=layout, cloud_index=True, **colour, **{**N_RIG, **N_GATES, **kw})


def check_oriented(spec, flow, unc, geometry, dest, seed=0, capacity_hit=False, plane_kw={}, colour_kw={}):
    """ppms_normals_egress writes the plane (the reference's bits), ppms_cloud_egress_normals reads it: counts, records, indices against the
    reference, poison everywhere else; the planes it read are as they were."""
    f0, n, left, top, h0, w0 = geometry
    colour = random_colour_plane(n, h0, w0, seed, spec.colour) if spec.colour else None
    want = expected(spec, flow, unc, *geometry, colour)
    plane = NormalsDest(spec.normals, n, h0, w0, **plane_kw)
    launch_normals(spec, plane.plane(), flow, unc, *geometry)
    assert same(plane.normals(n), want["normals"])
    keep = None
    if colour is not None:
        keep = ColourDest(n, h0, w0, **colour_kw)
        keep.plane.copy_(colour.to(DEV))
    before = plane.buf.clone()
    launch_cloud_normals(dest.struct(spec, n, h0, w0), plane.plane(), None if keep is None else keep.struct(spec.colour), flow, unc, *geometry)
    dest.check(n, want, capacity_hit)
    assert torch.equal(plane.buf, before) and (keep is None or keep.check(colour) is None)
    # condition of the test: point-valid pixels whose normal is invalid occur, so the second condition of a record decides somewhere
    points = OutputSpec(points="f32", uncertainty=None, Q=spec.Q, min_disp=spec.min_disp, max_uncertainty=spec.max_uncertainty, max_depth=spec.max_depth)
    T, _, H, W = flow.shape
    pv = ~points.reference(crop(flow, *geometry).cpu(), crop(upsampled(unc, H, W), *geometry).cpu())["points"][..., 2].isnan()
    counts = want["cloud_counts"]
    assert bool((pv.flatten(1).sum(1) > counts).any()) and bool((counts > 0).all())
    return want


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzn"), ("f16", "xyzn"), ("f32", "xyzrgbn")])
def test_oriented_cloud_frame_spans_three_workgroups(fmt, layout):
    """The A geometry: 37 rows of 7 runs = 259 runs per frame, three workgroups of 128 (the last with 3 runs).  Records ``lead`` bytes off the
    allocation's alignment, gaps between the frames, written from frame 1 of 4; the normals plane pitched."""
    flow, unc = state()
    es, C = (4 if fmt == "f32" else 2), (7 if layout == "xyzrgbn" else 6)
    dest = OrientedDest(fmt, C, 4, 37 * 50, first=1, gap=10 * es, index_gap=12, lead=es)
    want = check_oriented(oriented_spec(fmt, layout), flow, unc, A_CROP, dest, seed=831, plane_kw=dict(pitch_extra=3 * es, frame_gap=es),
                          colour_kw=dict(pitch_extra=12, frame_gap=20, lead=4))
    assert all(100 < c < 37 * 50 for c in want["cloud_counts"].tolist())


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzn"), ("f32", "xyzrgbn")])
def test_oriented_cloud_without_index_and_without_gates(fmt, layout):
    """No index; both gates off (NULL is accepted for unc); a whole frame of whole, 16-byte aligned runs: the 16-byte loads of the planes."""
    flow, unc = state(2, 32, 64, seed=9)
    spec = oriented_spec(fmt, layout, max_uncertainty=None, max_depth=None)
    geometry = (0, 2, 0, 0, 32, 64)
    C = 7 if layout == "xyzrgbn" else 6
    want = check_oriented(spec, flow, unc, geometry, OrientedDest(fmt, C, 2, 32 * 64, index=False), seed=832)
    # once more with unc = NULL
    colour = random_colour_plane(2, 32, 64, 832, spec.colour) if spec.colour else None
    plane = NormalsDest(fmt, 2, 32, 64)
    launch_normals(spec, plane.plane(), flow, unc, *geometry)
    keep = None
    if colour is not None:
        keep = ColourDest(2, 32, 64)
        keep.plane.copy_(colour.to(DEV))
    dest = OrientedDest(fmt, C, 2, 32 * 64, index=False)
    out, nrm = dest.struct(spec, 2, 32, 64), plane.plane()
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_cloud_egress_normals(flow.data_ptr(), None, 2, 32, 64, 0, 2, 0, 0, 32, 64, ctypes.byref(out), ctypes.byref(nrm),
                                                   None if keep is None else ctypes.byref(keep.struct(spec.colour)), L.stream_ptr()))
        torch.cuda.synchronize()
    dest.check(2, want)


@pytest.mark.parametrize("fmt,layout", [("f16", "xyzn"), ("f32", "xyzrgbn")])
def test_oriented_cloud_capacity_cuts_inside_the_second_workgroup(fmt, layout):
    flow, unc = state()
    spec = oriented_spec(fmt, layout)
    want = expected(spec, flow, unc, *A_CROP, random_colour_plane(2, 37, 50, 833, spec.colour) if spec.colour else None)
    # frame 0's second workgroup: runs 128 .. 255, pixels from row 18, column 16 (run 128 = 18 * 7 + 2) up to row 36, column 24 (run 256 = 36 * 7 + 4)
    first_wg, two_wgs = (int(want["cloud_index"][0].lt(p).sum()) for p in (18 * 50 + 16, 36 * 50 + 32))
    assert two_wgs - first_wg >= 2
    cut = first_wg + (two_wgs - first_wg) // 2
    check_oriented(spec, flow, unc, A_CROP, OrientedDest(fmt, 7 if layout == "xyzrgbn" else 6, 4, cut, first=1, gap=24, index_gap=8), seed=833,
                   capacity_hit=True)


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzrgbn"), ("f16", "xyzn")])
def test_oriented_cloud_more_workgroups_than_a_workgroup_has_threads(fmt, layout):
    """T = 1, 132 x 1024 uncropped: 128 runs per row, 16 896 runs, 132 workgroups of 128 in the frame -- more than a workgroup has threads, so the
    reduction that gives the last workgroups their base takes more than one block count per thread."""
    assert L.load().ppms_cloud_egress_normals_workspace(1, 132, 1024) == 132
    flow, unc = state(1, 132, 1024, seed=11)
    dest = OrientedDest(fmt, 7 if layout == "xyzrgbn" else 6, 1, 132 * 1024)
    check_oriented(oriented_spec(fmt, layout), flow, unc, (0, 1, 0, 0, 132, 1024), dest, seed=835)


def test_oriented_cloud_all_invalid_frames_write_nothing():
    flow, unc = state()
    spec = oriented_spec("f32", "xyzn", min_disp=1000.0)
    geometry = (0, 2, 1, 2, 27, 59)
    plane = NormalsDest("f32", 2, 27, 59)
    launch_normals(spec, plane.plane(), flow, unc, *geometry)
    assert bool(plane.normals(2).isnan().all())
    dest = OrientedDest("f32", 6, 2, 27 * 59, gap=8)
    launch_cloud_normals(dest.struct(spec, 2, 27, 59), plane.plane(), None, flow, unc, *geometry)
    want = expected(spec, flow, unc, *geometry)
    assert want["cloud_counts"].tolist() == [0, 0]
    dest.check(2, want)


# ---- 5. beside the old launches --------------------------------------------------------------------------------------------------------------------------
def test_launch_beside_the_planes_and_the_old_clouds_leaves_their_bits():
    """``_EgressCall.launch``: with ``normals=`` the older keys are the bits of the same spec without it; the "xyzn" / "xyzrgbn" clouds hold the
    points, the colour words and the "normals" plane's words at their indices; a hidden plane changes nothing but the keys."""
    from types import SimpleNamespace
    from ppmstereo_amd.engine import ScaleEngine
    from ppmstereo_amd.output import _EgressCall
    flow, unc = state()
    eng = SimpleNamespace(FLOW_OUT=flow, UNC=unc, T=3, h=16, w=16, shard=None)
    eng.egress = lambda *a: ScaleEngine.egress(eng, *a)
    kw = dict(disparity="u16", depth="u16", uncertainty="u8", points="f32", points_layout="xyzw", cloud="f32", cloud_index=True, colour="bgra8",
              focal_px=F, baseline=B, **N_RIG, **N_GATES)
    colour = random_colour_plane(2, 37, 50, 834).to(DEV)

    def launch(spec):
        call = _EgressCall(spec, A_CROP[2:], (1, 3))
        call.colour = colour
        return call.launch(eng)
    with torch.cuda.device(DEV):
        plain = launch(OutputSpec(cloud_layout="xyzrgb", **kw))
        beside = launch(OutputSpec(normals="f32", cloud_layout="xyzrgb", **kw))
        both = launch(OutputSpec(normals="f32", cloud_layout="xyzrgbn", **kw))
        hidden = launch(OutputSpec(normals="f32", normals_plane=False, colour_plane=False, cloud_layout="xyzrgbn", **kw))
        torch.cuda.synchronize()
    old = ["disparity", "depth", "uncertainties", "points"]
    rest = ["cloud", "cloud_counts", "cloud_index"]
    assert list(plain) == old + ["colour"] + rest and list(beside) == list(both) == old + ["normals", "colour"] + rest and list(hidden) == old + rest
    for other in (beside, both, hidden):
        assert same_results(other, plain, old)
    assert same(beside["normals"], both["normals"]) and tuple(both["normals"].shape) == (2, 37, 50, 3)
    assert torch.equal(beside["cloud_counts"], plain["cloud_counts"]) and torch.equal(both["cloud_counts"], hidden["cloud_counts"])
    nrm, words = both["normals"].view(torch.int32).reshape(2, -1, 3), colour.view(torch.int32).reshape(2, -1)
    for f in range(2):                                          # (rows past a frame's records are never written)
        count, kept = int(plain["cloud_counts"][f]), int(both["cloud_counts"][f])
        assert 0 < kept < count < 37 * 50
        assert torch.equal(beside["cloud"][f, :count].view(torch.int32), plain["cloud"][f, :count].view(torch.int32))
        index = both["cloud_index"][f, :kept].long()
        assert torch.equal(both["cloud_index"][f, :kept], hidden["cloud_index"][f, :kept])
        got = both["cloud"][f, :kept].view(torch.int32)
        assert torch.equal(got, hidden["cloud"][f, :kept].view(torch.int32))
        assert torch.equal(got[:, :3], both["points"][f].view(torch.int32).reshape(-1, 4)[index][:, :3])
        assert torch.equal(got[:, 3], words[f][index]) and torch.equal(got[:, 4:], nrm[f][index])
        assert not both["cloud"][f, :kept][:, 4:].isnan().any()


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------------------------------
def model_specs(ref_u, **kw):
    """(the spec with normals and the "xyzrgbn" cloud, the same spec without the new options): u16 / u8 planes and a cloud gated at the median of the
    default call's own uncertainty, so that valid and invalid pixels both occur whatever the procedural weights produce.  The jump gate is off: the
    procedural weights' disparities are no surface."""
    base = dict(disparity="u16", uncertainty="u8", cloud="f32", cloud_index=True, colour="bgra8", Q=OutputSpec.q_matrix(F, B, 125.0, 30.0),
                max_uncertainty=float(ref_u.abs().float().nanmedian()), **kw)
    return OutputSpec(normals="f32", normal_max_jump=None, cloud_layout="xyzrgbn", **base), OutputSpec(cloud_layout="xyzrgb", **base)


def against_reference(out, want, n, h, w):
    assert list(out) == ["disparity", "uncertainties", "normals", "colour", "cloud", "cloud_counts", "cloud_index"]
    assert tuple(out["normals"].shape) == (n, h, w, 3) and out["normals"].dtype == torch.float32
    assert same_results(out, want, ("disparity", "uncertainties", "normals")) and torch.equal(out["colour"], want["colour"])
    assert torch.equal(out["cloud_counts"], want["cloud_counts"]) and all(0 < c < h * w for c in out["cloud_counts"].tolist())
    for f in range(n):
        assert tuple(out["cloud"][f].shape) == (int(out["cloud_counts"][f]), 7) and torch.equal(out["cloud_index"][f], want["cloud_index"][f])
        assert torch.equal(out["cloud"][f].contiguous().view(torch.int32), want["cloud"][f].contiguous().view(torch.int32))


def test_model_several_windows_against_the_reference_on_the_float_path(model):
    """Three windows through the clip pipeline: the result equals ``reference`` applied to the float path's disparity and uncertainty and to
    ``colour_bytes`` of the left views; a spec without the new options returns its bits next to it."""
    from ppmstereo_amd.ppmstereo import window_plan
    assert len(window_plan(7, 4)) == 3
    video = rand_u8((7, 2, 3, 60, 250), 42)
    run = lambda **o: model.forward_batch_test({"stereo_video": video}, kernel_size=4, iters=2, **o)
    ref = run()
    spec, plain = model_specs(ref["uncertainties"])
    with torch.cuda.device(DEV):
        left = stereo_source("normals test", video.to(DEV)).float_views()[0]
    colour = colour_bytes(left, "bgra8").cpu()
    out = run(output=spec)
    assert out["normals"].is_pinned()
    against_reference(out, spec.reference(ref["disparity"], ref["uncertainties"], colour), 7, 60, 250)
    old = run(output=plain)
    assert same_results(out, old) and torch.equal(out["colour"], old["colour"]) and bool((old["cloud_counts"] >= out["cloud_counts"]).all())
    want_old = plain.reference(ref["disparity"], ref["uncertainties"], colour)
    assert all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(old["cloud"], want_old["cloud"]))
    hidden = OutputSpec(normals="f32", normal_max_jump=None, normals_plane=False, colour_plane=False, cloud_layout="xyzrgbn", cloud="f32", cloud_index=True,
                        colour="bgra8", Q=spec.Q, disparity="u16", uncertainty="u8", max_uncertainty=spec.max_uncertainty)
    got = run(output=hidden)
    assert list(got) == ["disparity", "uncertainties", "cloud", "cloud_counts", "cloud_index"] and same_results(got, out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got["cloud"], out["cloud"]))


def test_model_forward_returns_the_device_shapes(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 43).to(DEV), rand_u8((1, 3, 3, 64, 256), 44).to(DEV)
    rd, ru = model.forward(i1, i2, iters=2, test_mode=True)
    spec, _ = model_specs(ru.cpu())
    out = model.forward(i1, i2, iters=2, test_mode=True, output=spec, crop=(5, 3, 40, 200), frames=(1, 3))
    torch.cuda.synchronize()
    assert all(v.is_cuda and v.shape[0] == 1 for v in out.values())
    assert tuple(out["normals"].shape) == (1, 2, 40, 200, 3) and tuple(out["cloud"].shape) == (1, 2, 40 * 200, 7) and tuple(out["colour"].shape) == (1, 2, 40, 200, 4)
    want = spec.reference(rd[0, 1:3, :, 3:43, 5:205].cpu(), ru[0, 1:3, :, 3:43, 5:205].cpu(), colour_bytes(i1[0, 1:3, :, 3:43, 5:205].float(), "bgra8").cpu())
    host = {k: v[0].cpu() for k, v in out.items()}
    counts = host["cloud_counts"].tolist()
    host["cloud"], host["cloud_index"] = ([host[k][f, :c] for f, c in enumerate(counts)] for k in ("cloud", "cloud_index"))
    host["cloud_counts"] = host["cloud_counts"].long()
    against_reference(host, want, 2, 40, 200)


def test_model_refusals(model, monkeypatch):
    model_refuses(model, monkeypatch, OutputSpec(normals="f32", cloud="f32", cloud_layout="xyzn", Q=Q))
