"""CPU: the point-cloud back door.  ppms_scene_egress (ppms_disparity_egress plus a points plane reprojected with Q and the two gates) is part
of the C ABI, its ctypes binding has the header's argument list and struct layout, it refuses bad arguments before touching a device;
OutputSpec validates the new options and leaves a spec without them as it was; its ``reference`` is the arithmetic include/ppms.h states
(against float64 inside a derived bound, in fp32 exactly on the thresholds).  No device compute."""
import ctypes
import math

import pytest
import torch

from egress_util import CAL_700, _q, bad_ids, call_scene, grid_inputs, header_args, lib, refused  # noqa: F401  (lib: the fixture)

NAME = "ppms_scene_egress"


def test_declared_exported_bound_and_struct_layout(lib):
    from ppmstereo_amd import _lib as L
    for name in (NAME, "ppms_egress3d_struct_size"):
        assert header_args(name)
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.ppms_version() == 4
    args = header_args(NAME)
    assert args == header_args("ppms_disparity_egress")[:-2] + ["const ppms_egress3d* out", "void* stream"]
    ctype = {"int": ctypes.c_int, "const float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const ppms_egress3d*": ctypes.POINTER(L.Egress3D)}
    res, bound = L._SIGS[NAME]
    assert res is ctypes.c_int and bound == [ctype[a.rsplit(" ", 1)[0]] for a in args]
    assert header_args("ppms_egress3d_struct_size") == ["void"]
    assert lib.ppms_egress3d_struct_size() == ctypes.sizeof(L.Egress3D) == 112 + 32 + 64 + 8 + 8
    assert [(n, t) for n, t in L.Egress3D._fields_] == [("base", L.Egress), ("points", L.EgressPlane), ("q", ctypes.c_float * 16),
                                                       ("max_uncertainty", ctypes.c_float), ("max_depth", ctypes.c_float),
                                                       ("points_components", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    assert (L.Egress3D.base.offset, L.Egress3D.points.offset, L.Egress3D.q.offset, L.Egress3D.max_uncertainty.offset) == (0, 112, 144, 208)
    # the older entry point and its struct are as they were
    assert lib.ppms_egress_struct_size() == ctypes.sizeof(L.Egress) == 112 and ctypes.sizeof(L.EgressPlane) == 32
    assert [n for n, _ in L.Egress._fields_] == ["disparity", "depth", "uncertainty", "disp_scale", "fb", "depth_scale", "min_disp"]


# ---- argument refusal: egress_util's call (frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64, u16 / u16 / u8 planes) with an
# ---- "xyz" f32 points plane whose pitch (604) is wider than the row's 600 bytes, Q = identity and both gates on --------------------------------
NO_UNC_PLANE = ("disparity", "depth", "points")
nan, inf = math.nan, math.inf
# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [("no plane", dict(planes=())), ("null out", dict(null_out=True)),
       ("points.format", dict(points_format=2)), ("points.format", dict(points_format=3)), ("points.format", dict(points_format=-1)),
       ("points.format", dict(points_format=4)),
       ("points_components", dict(comps=2)), ("points_components", dict(comps=5)), ("points_components", dict(comps=0)),
       ("points.pitch", dict(points_pitch=596)), ("points.pitch", dict(comps=4, points_pitch=796)),                     # "xyzw" rows are 800 bytes
       ("points.pitch", dict(points_format=1, points_pitch=298)),                                                       # f16 rows are 300 bytes
       ("multiples of the 4-byte element", dict(points_pitch=602, points_frame_stride=37 * 602 + 2)),
       ("multiples of the 4-byte element", dict(points_frame_stride=37 * 604 + 2)),
       ("multiples of the 2-byte element", dict(points_format=1, points_pitch=301, points_frame_stride=37 * 301 + 1)),
       ("multiples of the 4-byte element", dict(points_ptr=0x600002)),
       ("points.frame_stride", dict(points_frame_stride=36 * 604 + 596)),                                               # frames overlap
       ("q[5]", dict(q=_q(5, nan))), ("q[15]", dict(q=_q(15, inf))), ("q[0]", dict(q=_q(0, -inf))), ("q[11]", dict(q=_q(11, nan), planes=("points",))),
       ("max_uncertainty", dict(max_uncertainty=nan)), ("max_uncertainty", dict(max_uncertainty=nan, planes=("disparity",))),
       ("max_depth", dict(max_depth=0.0)), ("max_depth", dict(max_depth=-1.0)), ("max_depth", dict(max_depth=nan)), ("max_depth", dict(max_depth=-inf)),
       ("null unc", dict(unc=0, planes=NO_UNC_PLANE)), ("null unc", dict(unc=0, planes=("depth",), max_depth=inf)),           # the gate on u
       ("null unc", dict(unc=0, planes=("points",), max_uncertainty=inf, comps=4, points_pitch=800, points_frame_stride=37 * 800)),                              # w of "xyzw"
       ("fb", dict(fb=0.0, planes=("depth",))), ("fb", dict(fb=nan, planes=("depth", "points"))),                        # a gated depth plane without fb
       ("min_disp", dict(min_disp=inf, planes=("points",))), ("min_disp", dict(min_disp=nan, planes=("disparity", "points"))),
       ("points.reserved", dict(points_reserved=1)), ("reserved", dict(reserved=1)),
       ("null flow_up", dict(flow=0, planes=("points",))),
       # the shared check, under this entry point's name
       ("disparity.format", dict(disparity_format=4)), ("uncertainty.format", dict(uncertainty_format=2)), ("crop", dict(pad_left=15)), ("crop", dict(H0=52)),
       ("multiples of 4", dict(W=62)), ("positive", dict(W0=0)), ("frame0", dict(frame0=2)), ("n_frames", dict(n_frames=0)),
       ("depth.pitch", dict(depth_pitch=99)), ("disparity.frame_stride", dict(disparity_frame_stride=36 * 102 + 98)), ("depth_scale", dict(depth_scale=0.0)),
       ("disp_scale", dict(disp_scale=0.0)), ("null flow_up", dict(unc=0)), ("multiples of the 2-byte element", dict(depth_ptr=0x400001))]


@pytest.mark.parametrize("about,bad", BAD, ids=bad_ids(BAD))
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    refused(lib, call_scene, "scene_egress", about, bad)


# ---- OutputSpec ------------------------------------------------------------------------------------------------------------------------
def test_output_spec_validation_of_the_new_options():
    from ppmstereo_amd.ppmstereo import OutputSpec
    Q = OutputSpec.q_matrix(700.0, 0.25, 19.5, 11.25)
    assert Q.dtype == torch.float64 and Q.tolist() == [[1, 0, 0, -19.5], [0, 1, 0, -11.25], [0, 0, 0, 700.0], [0, 0, 4.0, 0.0]]
    assert OutputSpec.q_matrix(700.0, 0.25, 19.5, 11.25, cx_right=20.0)[3].tolist() == [0, 0, 4.0, 2.0]
    for kw in (dict(points="f32"), dict(points="f16"),                                                             # points without Q
               dict(points="u16", Q=Q), dict(points="f64", Q=Q), dict(points="f32", Q=Q, points_layout="xyzi"), dict(points="f32", Q=Q, points_layout=None),
               dict(points="f32", Q=Q[:3]), dict(points="f32", Q=torch.full((4, 4), nan)), dict(points="f32", Q=[[inf] + [0.0] * 3] + [[0.0] * 4] * 3),
               dict(Q=[1.0, 0.0, 0.0, 0.0, 0.0, -inf] + [0.0] * 10),                                                 # (checked without points too)
               dict(max_depth=0.0), dict(max_depth=-3.0), dict(max_depth=nan), dict(max_depth=1e-60), dict(max_uncertainty=nan),
               dict(points="f32", Q=Q, min_disp=inf), dict(points="f32", Q=Q, min_disp=nan)):
        with pytest.raises(ValueError):
            OutputSpec(**kw)
    with pytest.raises(TypeError):
        OutputSpec("f32", None, "f32", 256.0, None, None, 1000.0, 2.0 ** -8, "f32")            # the new options are keyword only
    s = OutputSpec(points="f16", points_layout="xyzw", Q=Q.flatten().tolist(), max_uncertainty=0.1, max_depth=30.0, depth="u16", **CAL_700)
    assert list(s.formats().items()) == [("disparity", "f32"), ("depth", "u16"), ("uncertainties", "f32"), ("points", "f16")] and s.scene
    assert s.Q.dtype == torch.float32 and torch.equal(s.Q, Q.float()) and s.max_uncertainty == float(torch.tensor(0.1)) and s.max_depth == 30.0
    planes = s.empty(2, 5, 7, "cpu")
    assert [(k, tuple(v.shape), v.dtype) for k, v in planes.items()] == [("disparity", (2, 1, 5, 7), torch.float32), ("depth", (2, 1, 5, 7), torch.uint16),
                                                                          ("uncertainties", (2, 1, 5, 7), torch.float32), ("points", (2, 5, 7, 4), torch.float16)]
    st = s.scene_struct(planes)
    assert (st.points.ptr, st.points.frame_stride, st.points.pitch, st.points.format, st.points.reserved) == (planes["points"].data_ptr(), 5 * 7 * 8, 7 * 8, 1, 0)
    assert list(st.q) == Q.float().flatten().tolist() and (st.max_uncertainty, st.max_depth, st.points_components, st.reserved) == (s.max_uncertainty, 30.0, 4, 0)
    assert (st.base.depth.ptr, st.base.depth.pitch, st.base.fb, st.base.min_disp) == (planes["depth"].data_ptr(), 14, 175.0, 2.0 ** -8)
    xyz = OutputSpec(points="f32", Q=Q, uncertainty=None)
    assert list(xyz.formats()) == ["disparity", "points"] and tuple(xyz.empty(3, 4, 6, "cpu")["points"].shape) == (3, 4, 6, 3)
    st = xyz.scene_struct(xyz.empty(3, 4, 6, "cpu"))
    assert (st.points.frame_stride, st.points.pitch, st.points.format, st.points_components) == (4 * 6 * 12, 6 * 12, 0, 3)
    assert st.max_uncertainty == inf and st.max_depth == inf and st.base.uncertainty.ptr is None
    gates = OutputSpec(depth="f32", max_depth=50.0, **CAL_700)                                     # a gate alone takes the new entry point too
    assert gates.scene and list(gates.formats()) == ["disparity", "depth", "uncertainties"] and gates.scene_struct(gates.empty(1, 4, 4, "cpu")).points.ptr is None
    assert OutputSpec(max_depth=inf, max_uncertainty=inf).scene is False                       # +inf is "off"


def test_a_spec_without_the_new_options_is_as_before():
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import OutputSpec
    full = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54)
    assert not full.scene and not OutputSpec().scene and (full.points, full.Q, full.max_uncertainty, full.max_depth) == (None, None, None, None)
    assert list(full.formats().items()) == [("disparity", "u16"), ("depth", "u16"), ("uncertainties", "u8")]
    assert list(OutputSpec().formats().items()) == [("disparity", "f32"), ("uncertainties", "f32")]
    planes = full.empty(2, 5, 7, "cpu")
    assert [(k, tuple(v.shape), v.dtype) for k, v in planes.items()] == [("disparity", (2, 1, 5, 7), torch.uint16), ("depth", (2, 1, 5, 7), torch.uint16),
                                                                          ("uncertainties", (2, 1, 5, 7), torch.uint8)]
    st = full.struct(planes)
    assert type(st) is L.Egress and (st.depth.ptr, st.depth.frame_stride, st.depth.pitch, st.depth.format) == (planes["depth"].data_ptr(), 70, 14, 2)
    assert (st.disp_scale, st.fb, st.depth_scale, st.min_disp) == (256.0, full.fb, 1000.0, 2.0 ** -8)
    # and a spec WITH them hands ``struct`` the same planes and constants: ``scene_struct`` is built around it
    pts = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54, points="f32", Q=torch.eye(4))
    assert bytes(pts.struct(planes)) == bytes(st) == bytes(pts.scene_struct({**planes, "points": torch.empty(2, 5, 7, 3)}).base)


EPS = 4 * 2.0 ** -24


@pytest.mark.parametrize("layout", ["xyz", "xyzw"])
def test_reference_against_float64(layout):
    """Q = q_matrix(f, B, cx, cy) with cx_right = cx: the products with the matrix's zeros and ones are exact, so v_0 = x - cx, v_1 = y - cy (one
    rounding each: the exact sum of two fp32 numbers, rounded), v_2 = f (none) and v_3 = d * (1 / B) (one, with the fp32 entry 1 / B taken as given).
    X and Y carry three roundings -- the difference, the product, the division --, Z two: relative error at most 3 * 2^-24 to first order, bound
    4 * 2^-24.  Derived, not measured.  The gates compare exact inputs (d, u) with their thresholds, which float64 decides alike; Z and fb / d are
    computed, so the inputs are asserted to lie further than that bound, relatively, from max_depth."""
    from ppmstereo_amd.ppmstereo import OutputSpec
    f, B, cx, cy, min_disp, max_u, max_z = 700.0, 0.3, 19.5, 11.25, 0.5, 0.6, 20.0
    spec = OutputSpec(depth="f32", focal_px=f, baseline=B, min_disp=min_disp, points="f32", points_layout=layout, Q=OutputSpec.q_matrix(f, B, cx, cy),
                      max_uncertainty=max_u, max_depth=max_z)
    d, u = grid_inputs(min_disp=min_disp)
    got = spec.reference(d, u)
    C = 4 if layout == "xyzw" else 3
    assert tuple(got["points"].shape) == (2, 24, 40, C) and got["points"].dtype == torch.float32 and tuple(got["depth"].shape) == (2, 1, 24, 40)
    Q, D, U = spec.Q.double(), d.double().abs()[:, 0], u.double()[:, 0]
    x, y = torch.arange(40, dtype=torch.float64), torch.arange(24, dtype=torch.float64)[:, None]
    v3 = Q[3, 2] * D
    X, Y, Z = (x + Q[0, 3]) / v3, (y + Q[1, 3]) / v3, Q[2, 3] / v3
    valid_d, valid_u = D >= spec.min_disp, U <= spec.max_uncertainty
    far = lambda z: ((z / spec.max_depth - 1.0).abs() > 2 * EPS) | ~(valid_d & valid_u)
    Zd = spec.fb / D
    assert far(Z).all() and far(Zd).all(), "an input sits on the max_depth threshold: choose another seed"
    valid_z = (Z > 0) & (Z <= spec.max_depth)
    valid = valid_d & valid_u & valid_z
    # all four kinds of pixel are there
    assert valid.sum() > 100 and (valid_d & ~valid_u).sum() > 100 and (valid_d & valid_u & ~valid_z).sum() > 20
    assert (~valid_d & ~D.isnan()).sum() > 50 and D.isnan().sum() > 50 and (D == 0).sum() == 8
    p = got["points"].double()
    assert torch.equal(p[..., :3].isnan().all(-1), ~valid) and torch.equal(p[..., :3].isnan().any(-1), ~valid)
    for c, want in enumerate((X, Y, Z)):
        err = (p[..., c] - want).abs()[valid]
        assert (err <= EPS * want.abs()[valid]).all(), (c, (err / want.abs()[valid].clamp(min=1e-300)).max())
    if C == 4:
        assert torch.equal(got["points"][..., 3], u[:, 0])           # w: for valid and invalid points alike
    dvalid = valid_d & valid_u & (Zd <= spec.max_depth)
    z = got["depth"][:, 0].double()
    assert torch.equal(z.isinf(), ~dvalid) and ((z - Zd).abs()[dvalid] <= 2.0 ** -24 * Zd[dvalid]).all()
    # the gates never touch the other planes, and d of lower rank works: (H, W) -> (H, W, C)
    assert torch.equal(got["uncertainties"], u) and torch.equal(got["disparity"].isnan(), d.isnan())
    one = spec.reference(d[1, 0], u[1, 0])["points"]
    assert tuple(one.shape) == (24, 40, C) and torch.equal(one.isnan(), got["points"][1].isnan()) and torch.equal(one.nan_to_num(), got["points"][1].nan_to_num())
    with pytest.raises(ValueError):
        spec.reference(d[0, 0, 0], u[0, 0, 0])                         # no pixel grid
    with pytest.raises(ValueError):
        spec.reference(d)                                              # a gate on u, and no u


def test_reference_exactly_on_the_thresholds_and_f16_overflow():
    """f = 512, B = 0.5 (1 / B = 2, fb = 256: all exact), max_depth = 16: d = 16 gives Z = 512 / 32 = 16 and fb / d = 16 exactly -- valid, and d = 15.5 is not; u = max_uncertainty is valid, the next fp32 above is not; d = min_disp is valid (without the depth gate: its Z is far)."""
    from ppmstereo_amd.ppmstereo import OutputSpec
    Q = OutputSpec.q_matrix(512.0, 0.5, 1.0, 0.0)
    up = lambda v: float(torch.nextafter(torch.tensor(v), torch.tensor(inf)))
    down = lambda v: float(torch.nextafter(torch.tensor(v), torch.tensor(-inf)))
    kw = dict(depth="f32", focal_px=512.0, baseline=0.5, min_disp=0.25, points="f32", points_layout="xyzw", Q=Q, max_uncertainty=0.5)
    d = torch.tensor([[16.0, 15.5, 16.5, 16.0, 16.0, 0.25, down(0.25), -16.0]])
    u = torch.tensor([[0.5, 0.5, 0.5, up(0.5), down(0.5), 0.5, 0.5, -0.5]])
    got = OutputSpec(max_depth=16.0, **kw).reference(d, u)
    assert got["points"][0, :, 2].isnan().tolist() == [False, True, False, True, False, True, True, False]
    assert got["points"][0, 0].tolist() == [-1.0 / 32.0, 0.0, 16.0, 0.5] and got["points"][0, 7].tolist() == [6.0 / 32.0, 0.0, 16.0, 0.5]
    assert got["depth"][0].isinf().tolist() == [False, True, False, True, False, True, True, False] and got["depth"][0, 0] == 16.0
    assert torch.equal(got["points"][0, :, 3], u[0].abs())
    got = OutputSpec(**kw).reference(d, u)                                       # no depth gate: d = min_disp is valid, the next below is not
    assert got["points"][0, :, 2].isnan().tolist() == [False, False, False, True, False, False, True, False] and got["points"][0, 5, 2] == 1024.0
    assert got["depth"][0].isinf().tolist() == [False, False, False, True, False, False, True, False]
    # f16: the rounding to nearest even of the fp32 value; 65520 and above overflow to inf, an invalid point stays NaN
    d = torch.tensor([[2.0 ** -8, 256.0 / 65519.0, 256.0 / 65521.0, 1.0, nan, 300.0]])      # Z = 256 / d: 65536, 65519 (-> 65504), 65521 (-> inf)
    h = OutputSpec(points="f16", Q=Q, min_disp=2.0 ** -8, uncertainty=None).reference(d)
    s = OutputSpec(points="f32", Q=Q, min_disp=2.0 ** -8, uncertainty=None).reference(d)
    assert h["points"].dtype == torch.float16 and tuple(h["points"].shape) == (1, 6, 3)
    assert s["points"][0, 0].tolist() == [-128.0, 0.0, 65536.0] and h["points"][0, 0].tolist() == [-128.0, 0.0, inf]
    assert 65518.0 < s["points"][0, 1, 2] < 65520.0 < s["points"][0, 2, 2] < 65522.0 and h["points"][0, 1:3, 2].tolist() == [65504.0, inf]
    assert torch.equal(h["points"].isnan(), s["points"].isnan()) and h["points"][0, 4].isnan().all() and not h["points"][0, [0, 1, 2, 3, 5]].isnan().any()
    assert torch.equal(h["points"].nan_to_num(), s["points"].to(torch.float16).nan_to_num())
