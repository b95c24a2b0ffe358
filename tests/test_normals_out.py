"""CPU: surface normals out.  ppms_normals_egress and ppms_cloud_egress_normals are part of the C ABI, their ctypes bindings have the header's
argument lists and struct layout, they refuse bad arguments before touching a device; OutputSpec validates the new options, orders the new keys and
fills the new struct; its ``reference`` -- the definition the kernels are tested against -- has the properties of a normal on the surface state, agrees
with the stencil restated in float64, and makes the oriented clouds of its own points, normals and colour words.  No device compute."""
import ctypes
import math
import os
import re

import pytest
import torch

from colour_util import random_colour_plane
from egress_util import CAL_700, ROOT, _q, bad_ids, header_args, lib, refused  # noqa: F401  (lib: the fixture)
from normals_util import (A_CROP, N_GATES, N_RIG, Q_REVERSED, call_cloud_normals, call_normals, crop, every_kind, stencil64, stencil_kinds,
                          surface_state)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec

nan, inf = math.nan, math.inf
Q = N_RIG["Q"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_declared_exported_bound_and_struct_layout(lib):
    names = ("ppms_normals_egress", "ppms_normals_struct_size", "ppms_cloud_egress_normals", "ppms_cloud_egress_normals_workspace")
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.ppms_version() == 4
    ctype = {"int": ctypes.c_int, "const float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const ppms_cloud*": ctypes.POINTER(L.Cloud),
             "const ppms_normals*": ctypes.POINTER(L.Normals), "const ppms_egress_plane*": ctypes.POINTER(L.EgressPlane)}
    head = header_args("ppms_scene_egress")[:-2]
    for name, tail in (("ppms_normals_egress", ["const ppms_normals* out", "void* stream"]),
                       ("ppms_cloud_egress_normals", ["const ppms_cloud* out", "const ppms_egress_plane* normals", "const ppms_egress_plane* colour", "void* stream"])):
        args = header_args(name)
        res, bound = L._SIGS[name]
        assert args == head + tail and res is ctypes.c_int and bound == [ctype[a.rsplit(" ", 1)[0]] for a in args], name
    assert header_args("ppms_normals_struct_size") == ["void"] and L._SIGS["ppms_normals_struct_size"] == (ctypes.c_int, [])
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppms.h")).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+ppms_cloud_egress_normals_workspace\s*\(\s*int n_frames,\s*int H0,\s*int W0\s*\)\s*;", src)
    assert L._SIGS["ppms_cloud_egress_normals_workspace"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    body = re.search(r"typedef struct ppms_normals \{(.*?)\} ppms_normals;", src, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == [n for n, _ in L.Normals._fields_] == ["normals", "q", "min_disp", "max_uncertainty", "max_depth", "max_jump", "reserved"]
    assert lib.ppms_normals_struct_size() == ctypes.sizeof(L.Normals) == 120
    assert (L.Normals.q.offset, L.Normals.min_disp.offset, L.Normals.max_jump.offset, L.Normals.reserved.offset) == (32, 96, 108, 112)
    # the older doors are as they were
    assert lib.ppms_cloud_struct_size() == ctypes.sizeof(L.Cloud) == 152 and lib.ppms_egress3d_struct_size() == ctypes.sizeof(L.Egress3D) == 224


def test_workspace_entries(lib):
    """One entry per workgroup of 128 runs of 8 pixels of one frame: twice ppms_cloud_egress's, whose query is as it was."""
    ws, old = lib.ppms_cloud_egress_normals_workspace, lib.ppms_cloud_egress_workspace
    assert ws(2, 37, 50) == 2 * 3 and ws(1, 16, 64) == 1 and ws(3, 16, 64) == 3 and ws(1, 16, 65) == 2 and ws(1, 516, 1024) == 516
    assert ws(1, 1, 1) == 1 and ws(0, 8, 8) == 0 and ws(1, 0, 8) == 0 and ws(1, 65536, 32768) == 0
    assert old(2, 37, 50) == 4 and old(1, 516, 1024) == 258


# ---- argument refusal: egress_util's geometry (frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64) ------------------------------------
GEOMETRY_BAD = [("crop", dict(pad_left=15)), ("crop", dict(H0=52)), ("crop", dict(pad_top=-1)), ("multiples of 4", dict(W=62)), ("positive", dict(W0=0)),
                ("positive", dict(T=0)), ("frame0", dict(frame0=2)), ("frame0", dict(frame0=-1)), ("n_frames", dict(n_frames=0))]
REPROJECTION_BAD = [("q[5]", dict(q=_q(5, nan))), ("q[15]", dict(q=_q(15, inf))), ("min_disp", dict(min_disp=inf)), ("min_disp", dict(min_disp=nan)),
                    ("max_uncertainty", dict(max_uncertainty=nan)), ("max_depth", dict(max_depth=0.0)), ("max_depth", dict(max_depth=nan)),
                    ("null unc", dict(unc=0)), ("null flow_up", dict(flow=0)), ("reserved", dict(reserved=1))]
PLANE_BAD = [("null normals plane", dict(ptr=0)), ("normals.format", dict(format=2)), ("normals.format", dict(format=3)), ("normals.format", dict(format=4)),
             ("normals.format", dict(format=-1)), ("normals.pitch", dict(pitch=596)), ("normals.pitch", dict(format=1, pitch=298)),
             ("normals.frame_stride", dict(frame_stride=36 * 604 + 596)), ("normals.reserved", dict(plane_reserved=1)),
             ("multiples of the 4-byte element", dict(ptr=0x300002)), ("multiples of the 4-byte element", dict(pitch=606, frame_stride=37 * 606)),
             ("multiples of the 2-byte element", dict(format=1, ptr=0x300001))]
BAD_NORMALS = ([("null out", dict(null_out=True))] + PLANE_BAD + [("max_jump", dict(max_jump=0.0)), ("max_jump", dict(max_jump=-0.05)),
               ("max_jump", dict(max_jump=nan)), ("max_jump", dict(max_jump=-inf))] + REPROJECTION_BAD + GEOMETRY_BAD)


@pytest.mark.parametrize("about,bad", BAD_NORMALS, ids=bad_ids(BAD_NORMALS))
def test_normals_egress_refuses(lib, about, bad):
    refused(lib, call_normals, "normals_egress", about, bad)


_plane = lambda bad: dict(normals={("reserved" if k == "plane_reserved" else k): v for k, v in bad.items()})
BAD_CLOUD = ([("null out", dict(null_out=True)), ("null records", dict(records=0)), ("null counts", dict(counts=0)),
              ("components", dict(components=5)), ("components", dict(components=8)), ("components", dict(components=3)), ("components", dict(components=4)),
              ("format", dict(format=2)), ("capacity", dict(capacity=0)), ("frame_stride", dict(frame_stride=23996)),
              ("frame_stride", dict(components=7, colour={}, frame_stride=27996)), ("index_frame_stride", dict(index_frame_stride=3996)),
              ("block_counts", dict(block_counts=0)), ("ppms_cloud_egress_normals_workspace", dict(block_counts_len=5)),       # (ppms_cloud_egress's 4 are too few)
              ("ppms_cloud_egress_normals_workspace", dict(block_counts_len=4)),
              ("null normals plane", dict(null_normals=True))]
             + [(about, _plane(bad)) for about, bad in PLANE_BAD if "format=1" not in str(bad) and bad.get("format") != 1]
             + [("differs from the records' format", dict(normals=dict(format=1, pitch=302, frame_stride=37 * 302))),
                ("differs from the records' format", dict(format=1, frame_stride=12016)),
                ("takes no colour plane", dict(colour={})),                                                                      # superfluous
                ("null colour plane", dict(components=7, frame_stride=28016)), ("null colour plane", dict(components=7, frame_stride=28016, colour=dict(ptr=0))),
                ("colour.format", dict(components=7, frame_stride=28016, colour=dict(format=0))),
                ("colour.pitch", dict(components=7, frame_stride=28016, colour=dict(pitch=196))),
                ("must be PPMS_FMT_F32", dict(components=7, format=1, frame_stride=14016, colour={}, normals=dict(format=1, pitch=302, frame_stride=37 * 302)))]
             + [(a, b) for a, b in REPROJECTION_BAD] + GEOMETRY_BAD)


@pytest.mark.parametrize("about,bad", BAD_CLOUD, ids=[f"{i}-" + s for i, s in enumerate(bad_ids([(a, {k: v for k, v in b.items() if not isinstance(v, dict)}) for a, b in BAD_CLOUD]))])
def test_cloud_egress_normals_refuses(lib, about, bad):
    refused(lib, call_cloud_normals, "cloud_egress_normals", about, bad)


# ---- OutputSpec ------------------------------------------------------------------------------------------------------------------------------
def test_output_spec_validation_of_the_new_options():
    for kw in (dict(normals="f32"), dict(normals="f16"),                                                               # normals without Q
               dict(normals="u16", Q=Q), dict(normals="f64", Q=Q), dict(normals=True, Q=Q),
               dict(normals="f32", Q=Q, min_disp=inf), dict(normals="f32", Q=Q, min_disp=nan),
               dict(normals="f32", Q=Q, normal_max_jump=0.0), dict(normals="f32", Q=Q, normal_max_jump=-0.05), dict(normals="f32", Q=Q, normal_max_jump=nan),
               dict(Q=Q, normal_max_jump=0.1), dict(Q=Q, normal_max_jump=None), dict(Q=Q, normal_max_jump=inf),              # the normals' option without normals
               dict(Q=Q, points="f32", points_layout="xyzn"), dict(Q=Q, points="f32", normals="f32", points_layout="xyzn"),  # points_layout does not grow
               dict(Q=Q, cloud_layout="xyzn"), dict(Q=Q, normals="f32", cloud_layout="xyzn"),                                # no cloud
               dict(Q=Q, cloud="f32", cloud_layout="xyzn"), dict(Q=Q, cloud="f32", cloud_layout="xyzn", normals="f16"),       # normals in the cloud's format
               dict(Q=Q, cloud="f16", cloud_layout="xyzn", normals="f32"),
               dict(Q=Q, cloud="f32", cloud_layout="xyzrgbn", normals="f32"),                                              # no colour
               dict(Q=Q, cloud="f16", cloud_layout="xyzrgbn", normals="f16", colour="bgra8"),                               # the colour word needs f32
               dict(Q=Q, cloud="f32", cloud_layout="xyzrgbn", colour="bgra8"), dict(Q=Q, cloud="f32", cloud_layout="xyzrgbn", colour="bgra8", normals="f16"),
               dict(Q=Q, normals="f32", normals_plane=False), dict(Q=Q, normals="f32", cloud="f32", normals_plane=False),     # only with the two layouts
               dict(Q=Q, normals="f32", cloud="f32", cloud_layout="xyzrgb", colour="bgra8", normals_plane=False),
               dict(Q=Q, normals="f32", cloud="f32", cloud_layout="xyzn", normals_plane=0), dict(Q=Q, normals="f32", cloud="f32", cloud_layout="xyzn", colour_plane=False)):
        with pytest.raises(ValueError):
            OutputSpec(**kw)
    with pytest.raises(TypeError):
        OutputSpec("f32", None, "f32", 256.0, None, None, 1000.0, 2.0 ** -8, None, "xyz", Q, None, None, None, "xyz", False, None, None, True, "f32")
    s = OutputSpec(normals="f16", Q=Q)
    assert (s.normals, s.normal_max_jump, s.normals_plane, s.scene) == ("f16", float(torch.tensor(0.05)), True, False)
    assert OutputSpec(normals="f32", Q=Q, normal_max_jump=None).normal_max_jump is None and OutputSpec(normals="f32", Q=Q, normal_max_jump=inf).normal_max_jump is None
    old = OutputSpec(Q=Q, points="f32")
    assert (old.normals, old.normal_max_jump, old.normals_plane) == (None, float(torch.tensor(0.05)), True) and "normals" not in old.formats()
    assert OutputSpec(Q=Q, normals="f32", cloud="f32", cloud_layout="xyzrgbn", colour="rgba8", colour_plane=False, normals_plane=False).cloud_components == 7


def test_formats_empty_and_the_struct():
    s = OutputSpec(depth="u16", points="f16", points_layout="xyzw", normals="f32", colour="bgra8", cloud="f32", cloud_layout="xyzrgbn", cloud_index=True,
                   cloud_capacity=9, Q=Q, normal_max_jump=0.125, max_uncertainty=0.5, max_depth=30.0, **CAL_700)
    assert list(s.formats().items()) == [("disparity", "f32"), ("depth", "u16"), ("uncertainties", "f32"), ("points", "f16"), ("normals", "f32"),
                                         ("colour", "bgra8"), ("cloud", "f32"), ("cloud_counts", "i32"), ("cloud_index", "i32")]
    planes = s.empty(2, 5, 7, "cpu")
    assert [(k, tuple(v.shape), v.dtype) for k, v in planes.items()][3:] == [
        ("points", (2, 5, 7, 4), torch.float16), ("normals", (2, 5, 7, 3), torch.float32), ("colour", (2, 5, 7, 4), torch.uint8),
        ("cloud", (2, 9, 7), torch.float32), ("cloud_counts", (2,), torch.int32), ("cloud_index", (2, 9), torch.int32)]
    st = s.normals_struct(planes)
    assert type(st) is L.Normals and (st.normals.ptr, st.normals.frame_stride, st.normals.pitch, st.normals.format, st.normals.reserved) == (
        planes["normals"].data_ptr(), 5 * 7 * 12, 7 * 12, L.FMT_F32, 0)
    assert list(st.q) == Q.float().flatten().tolist() and (st.min_disp, st.max_uncertainty, st.max_depth, st.max_jump, st.reserved) == (2.0 ** -8, 0.5, 30.0, 0.125, 0)
    cl = s.cloud_struct(planes, torch.empty(4, dtype=torch.int32))
    assert (cl.frame_stride, cl.capacity, cl.format, cl.components) == (9 * 28, 9, L.FMT_F32, 7)
    # f16 beside an "xyzn" f16 cloud; both planes hidden; the gates off
    h = OutputSpec(normals="f16", normals_plane=False, cloud="f16", cloud_layout="xyzn", Q=Q, normal_max_jump=None)
    assert list(h.formats()) == ["disparity", "uncertainties", "cloud", "cloud_counts"] and h.cloud_components == 6
    planes = h.empty(3, 4, 6, "cpu")
    assert "normals" not in planes and tuple(planes["cloud"].shape) == (3, 24, 6) and planes["cloud"].dtype == torch.float16
    st = h.normals_struct({"normals": torch.empty(3, 4, 6, 3, dtype=torch.float16)})
    assert (st.normals.frame_stride, st.normals.pitch, st.normals.format) == (4 * 6 * 6, 6 * 6, L.FMT_F16)
    assert (st.max_uncertainty, st.max_depth, st.max_jump) == (inf, inf, inf) and h.normals_struct({}).normals.ptr is None


def test_a_spec_without_the_new_options_is_as_before():
    kw = dict(disparity="u16", depth="u16", uncertainty="u8", points="f16", points_layout="xyzw", Q=Q, max_uncertainty=0.7, max_depth=12.0, colour="rgba8",
              cloud="f32", cloud_layout="xyzrgb", cloud_index=True, **CAL_700)
    old, new = OutputSpec(**kw), OutputSpec(normals="f32", **kw)
    planes = new.empty(2, 5, 7, "cpu")
    assert [k for k in planes if k != "normals"] == list(old.empty(2, 5, 7, "cpu"))
    ws = torch.empty(4, dtype=torch.int32)
    assert bytes(old.scene_struct(planes)) == bytes(new.scene_struct(planes)) and bytes(old.cloud_struct(planes, ws)) == bytes(new.cloud_struct(planes, ws))
    flow, _ = surface_state()
    d = crop(flow, *A_CROP)
    u = torch.rand(d.shape, generator=torch.Generator().manual_seed(3))
    colour = random_colour_plane(2, 37, 50, 5, "rgba8")
    a, b = old.reference(d, u, colour), new.reference(d, u, colour)
    assert list(a) == ["disparity", "depth", "uncertainties", "points", "colour", "cloud", "cloud_index", "cloud_counts"]
    assert list(b) == list(a)[:4] + ["normals"] + list(a)[4:]
    bits = lambda t: t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.element_size() > 1 else t
    for k in a:
        for x, y in zip(*((v if isinstance(v, list) else [v]) for v in (a[k], b[k]))):
            assert x.dtype == y.dtype and torch.equal(bits(x.contiguous()), bits(y.contiguous())), k


# ---- reference: the definition on the surface state ------------------------------------------------------------------------------------------------
def surface(noise=0.02, seed=5):
    """(d, u): the A crop of the surface state -- frames [1, 3), 37 x 50 at (13, 7) -- and a random full-resolution uncertainty of that shape."""
    flow, _ = surface_state(noise=noise, seed=seed)
    d = crop(flow, *A_CROP)
    return d, torch.rand(d.shape, generator=torch.Generator().manual_seed(seed + 1))


@pytest.mark.parametrize("gates", [dict(), dict(max_depth=12.0), N_GATES], ids=["no_gate", "max_depth", "both_gates"])
def test_reference_normals_are_unit_face_the_camera_and_cover_every_stencil_kind(gates):
    spec = OutputSpec(points="f32", normals="f32", **N_RIG, **gates)
    d, u = surface()
    out = spec.reference(d, u)
    P, n = out["points"], out["normals"]
    assert list(out) == ["disparity", "uncertainties", "points", "normals"] and tuple(n.shape) == (2, 37, 50, 3) and n.dtype == torch.float32
    valid = ~n[..., 0].isnan()
    assert torch.equal(n.isnan().any(-1), n.isnan().all(-1))                                # NaN in all three components or in none
    assert not (valid & P[..., 2].isnan()).any()                                            # an invalid centre gives NaN
    table, stencil_valid = stencil_kinds(spec, d, u)
    assert every_kind(table, 4), table.tolist()                                             # condition of the tests on the GPU side too
    assert torch.equal(valid, stencil_valid)
    if not gates:
        assert int(valid.sum()) == 3280 and int((~P[..., 2].isnan() & ~valid).sum()) > 0    # valid points without a normal occur
    length = n[valid].double().pow(2).sum(-1).sqrt()
    assert float((length - 1.0).abs().max()) <= 4 * 2.0 ** -24                              # three roundings of products, a sum, sqrt, the division: a few ulp
    assert float((n[valid].double() * P[valid].double()).sum(-1).max()) <= 0.0              # towards the origin
    # f16 is the rounding of the fp32 value; a hidden plane leaves the key out
    half = OutputSpec(normals="f16", **N_RIG, **gates).reference(d, u)["normals"]
    assert half.dtype == torch.float16 and torch.equal(half.isnan(), n.isnan()) and torch.equal(half[valid], n[valid].to(torch.float16))


def test_reference_one_row_and_one_column_have_no_normal():
    d, u = surface()
    spec = OutputSpec(normals="f32", **N_RIG)
    for cut in (d[:, :, 5:6, :], d[:, :, :, 9:10]):
        n = OutputSpec(normals="f32", uncertainty=None, **N_RIG).reference(cut)["normals"]
        assert tuple(n.shape) == (2, *cut.shape[-2:], 3) and bool(n.isnan().all())
    # two rows: a one-sided vertical tangent everywhere, so normals exist
    assert int((~spec.reference(d[:, :, 5:7, :], u[:, :, 5:7, :])["normals"][..., 0].isnan()).sum()) > 20


def test_reference_reversed_baseline_negates_every_normal_and_all_took_the_flip():
    d, _ = surface()
    kw = dict(normals="f32", uncertainty=None, min_disp=0.25)
    n = OutputSpec(Q=Q, **kw).reference(d)["normals"]
    r = OutputSpec(Q=Q_REVERSED, **kw).reference(d)["normals"]
    valid = ~n[..., 0].isnan()
    assert int(valid.sum()) == 3280 and torch.equal(valid, ~r[..., 0].isnan()) and torch.equal(r[valid], -n[valid])
    # which side the cross product came out on, from the float64 restatement: none flipped with Q, all with the reversed baseline
    flipped, flipped_r = (stencil64(OutputSpec(Q=q, **kw), d)[1][:, 0] for q in (Q, Q_REVERSED))
    assert not flipped[valid].any() and bool(flipped_r[valid].all())


@pytest.mark.parametrize("gates", [dict(), dict(max_depth=12.0)], ids=["no_gate", "max_depth"])
def test_reference_against_the_stencil_in_float64(gates):
    """The noise-free surface (holes and signs as ever): the fp32 definition against its float64 restatement from the disparity on.  Worst angle
    observed: 2.26e-5 rad (both cases, seed 5) -- the points' fp32 rounding, about 1e-6 of a unit in X and Z against neighbour differences of 0.015;
    asserted at four times that, which covers other seeds.  It checks the definition, not the kernel."""
    d, _ = surface(noise=0.0)
    spec = OutputSpec(normals="f32", uncertainty=None, **N_RIG, **gates)
    got, (want, _) = spec.reference(d)["normals"].double(), stencil64(spec, d)
    want = want[:, 0]
    valid = ~got[..., 0].isnan()
    assert torch.equal(valid, ~want[..., 0].isnan()) and int(valid.sum()) > 3000
    angle = torch.asin(torch.linalg.cross(got[valid], want[valid]).norm(dim=-1).clamp(max=1.0))
    print("worst angle", float(angle.max()))
    assert float(angle.max()) <= 4 * 2.26e-5 and float((got[valid] * want[valid]).sum(-1).min()) > 0.99


@pytest.mark.parametrize("fmt,layout", [("f32", "xyzn"), ("f16", "xyzn"), ("f32", "xyzrgbn")])
def test_reference_oriented_cloud_is_its_own_points_normals_and_colour_words(fmt, layout):
    colour_kw = dict(colour="bgra8") if layout == "xyzrgbn" else {}
    spec = OutputSpec(points=fmt, normals=fmt, cloud=fmt, cloud_layout=layout, cloud_index=True, cloud_capacity=5, **colour_kw, **N_RIG, **N_GATES)
    d, u = surface()
    colour = random_colour_plane(2, 37, 50, 821) if colour_kw else None
    got = spec.reference(d, u, colour)
    pts, nrm = got["points"], got["normals"]
    point_valid, valid = ~pts[..., 2].float().isnan(), ~nrm[..., 0].float().isnan()
    assert int((point_valid & ~valid).sum()) > 50 and not (valid & ~point_valid).any()      # kept iff the point AND the normal are valid
    assert got["cloud_counts"].tolist() == valid.flatten(1).sum(1).tolist() and min(got["cloud_counts"].tolist()) > 5
    C = 7 if layout == "xyzrgbn" else 6
    for fr in range(2):
        cloud, index = got["cloud"][fr], got["cloud_index"][fr]
        assert cloud.dtype == pts.dtype and tuple(cloud.shape) == (int(got["cloud_counts"][fr]), C)
        assert torch.equal(index, valid[fr].flatten().nonzero().flatten().to(torch.int32))
        bits = lambda t: t.contiguous().view(torch.int32 if fmt == "f32" else torch.int16)
        assert torch.equal(bits(cloud[:, :3]), bits(pts[fr][valid[fr]])) and torch.equal(bits(cloud[:, -3:]), bits(nrm[fr][valid[fr]]))
        if C == 7:
            assert torch.equal(bits(cloud[:, 3]), colour[fr].view(torch.int32).flatten()[index.long()])
    # the plane hidden: the same cloud, no "normals" key; the "xyz" cloud beside normals keeps every valid point
    hidden = OutputSpec(normals=fmt, normals_plane=False, cloud=fmt, cloud_layout=layout, **colour_kw, **N_RIG, **N_GATES).reference(d, u, colour)
    assert "normals" not in hidden and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(hidden["cloud"], got["cloud"]))
    plain = OutputSpec(normals=fmt, cloud=fmt, **N_RIG, **N_GATES).reference(d, u)
    assert plain["cloud_counts"].tolist() == point_valid.flatten(1).sum(1).tolist()
    with pytest.raises(ValueError):
        OutputSpec(normals="f32", **N_RIG, max_uncertainty=0.5).reference(d)                 # the gate, and no u
