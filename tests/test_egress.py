"""CPU: the quantised back door.  ppms_disparity_egress (the 1/4 scale's last iteration -> cropped, converted output planes of the kept
frames) is part of the C ABI, its ctypes binding has the header's argument list and struct size, it refuses bad arguments before touching a
device; OutputSpec validates and its ``reference`` is the arithmetic include/ppms.h states (against float64 away from ties, in fp32 at ties
and edge values); egress_plan is the window-to-slice arithmetic of forward_batch_test(output=...).  No device compute."""
import ctypes
import math

import pytest
import torch

from egress_util import call_disparity, header_args, lib, refused  # noqa: F401  (lib: the fixture)

NAME = "ppms_disparity_egress"


def test_declared_exported_bound_and_abi_version_unchanged(lib):
    from ppmstereo_amd import _lib as L
    for name in (NAME, "ppms_egress_struct_size"):
        assert header_args(name)
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.ppms_version() == 4
    args = header_args(NAME)
    assert args == ["const float* flow_up", "const float* unc", "int T", "int H", "int W", "int frame0", "int n_frames", "int pad_left", "int pad_top",
                    "int H0", "int W0", "const ppms_egress* out", "void* stream"]
    ctype = {"int": ctypes.c_int, "const float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const ppms_egress*": ctypes.POINTER(L.Egress)}
    res, bound = L._SIGS[NAME]
    assert res is ctypes.c_int and bound == [ctype[a.rsplit(" ", 1)[0]] for a in args]
    assert header_args("ppms_egress_struct_size") == ["void"]
    assert lib.ppms_egress_struct_size() == ctypes.sizeof(L.Egress) == 112 and ctypes.sizeof(L.EgressPlane) == 32
    assert [n for n, _ in L.EgressPlane._fields_] == ["ptr", "frame_stride", "pitch", "format", "reserved"]
    assert [n for n, _ in L.Egress._fields_] == ["disparity", "depth", "uncertainty", "disp_scale", "fb", "depth_scale", "min_disp"]
    assert (L.FMT_F32, L.FMT_F16, L.FMT_U16, L.FMT_U8) == (0, 1, 2, 3)


# ---- argument refusal: egress_util's call (frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64, u16 / u16 / u8 planes) ----------------
# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [("no plane", dict(planes=())), ("null out", dict(null_out=True)),
       ("disparity.format", dict(disparity_format=4)), ("depth.format", dict(depth_format=-1)), ("uncertainty.format", dict(uncertainty_format=7)),
       ("disparity.format", dict(disparity_format=3)), ("depth.format", dict(depth_format=3)),                 # u8 is the uncertainty's alone
       ("uncertainty.format", dict(uncertainty_format=2)), ("uncertainty.format", dict(uncertainty_format=1)),  # u16 / f16 are not
       ("crop", dict(pad_left=15)), ("crop", dict(pad_top=28)), ("crop", dict(pad_left=-1)), ("crop", dict(pad_top=-1)), ("crop", dict(H0=52)),
       ("crop", dict(W0=58)), ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62)), ("positive", dict(H0=0)), ("positive", dict(W0=0)),
       ("frame0", dict(frame0=2)), ("frame0", dict(frame0=-1)), ("frame0", dict(n_frames=3)), ("n_frames", dict(n_frames=0)), ("n_frames", dict(n_frames=-2)),
       ("disparity.pitch", dict(disparity_pitch=98)), ("depth.pitch", dict(depth_pitch=99)), ("uncertainty.pitch", dict(uncertainty_pitch=49)),
       ("depth.pitch", dict(depth_format=0, depth_pitch=196)),                                                  # f32 rows are 200 bytes
       ("disparity.frame_stride", dict(disparity_frame_stride=36 * 102 + 98)),                                   # frames overlap
       ("fb", dict(fb=0.0)), ("fb", dict(fb=-1.0)), ("fb", dict(fb=math.nan)), ("depth_scale", dict(depth_scale=0.0)), ("depth_scale", dict(depth_scale=-1000.0)),
       ("min_disp", dict(min_disp=math.inf)), ("min_disp", dict(min_disp=math.nan)),
       ("disp_scale", dict(disp_scale=0.0)), ("disp_scale", dict(disp_scale=-256.0)),
       ("null flow_up", dict(flow=0)), ("null flow_up", dict(unc=0)),
       ("disparity.reserved", dict(disparity_reserved=1)),
       ("multiples of the 2-byte element", dict(depth_ptr=0x400001)), ("multiples of the 2-byte element", dict(disparity_pitch=103, disparity_frame_stride=37 * 103 + 1))]


@pytest.mark.parametrize("about,bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for _, b in BAD])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    refused(lib, call_disparity, "disparity_egress", about, bad)


# ---- OutputSpec ------------------------------------------------------------------------------------------------------------------------
def test_output_spec_validation():
    from ppmstereo_amd.ppmstereo import OutputSpec
    s = OutputSpec()
    assert (s.disparity, s.depth, s.uncertainty, s.disp_scale, s.depth_scale) == ("f32", None, "f32", 256.0, 1000.0)
    assert list(s.formats()) == ["disparity", "uncertainties"]
    full = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54)
    assert list(full.formats().items()) == [("disparity", "u16"), ("depth", "u16"), ("uncertainties", "u8")]
    assert full.fb == float(torch.tensor(721.5377, dtype=torch.float32) * torch.tensor(0.54, dtype=torch.float32))
    assert list(OutputSpec(uncertainty=None).formats()) == ["disparity"]
    for kw in (dict(disparity="u8"), dict(disparity=None), dict(disparity="f64"), dict(depth="u8"), dict(uncertainty="u16"), dict(uncertainty="f16"),
               dict(depth="u16"), dict(depth="f32", focal_px=700.0), dict(depth="f16", baseline=0.5),                    # depth without both constants
               dict(depth="u16", focal_px=0.0, baseline=0.5), dict(depth="u16", focal_px=700.0, baseline=-0.5),
               dict(depth="u16", focal_px=700.0, baseline=0.5, depth_scale=0.0), dict(depth="f32", focal_px=700.0, baseline=0.5, min_disp=math.inf),
               dict(depth="f32", focal_px=700.0, baseline=0.5, min_disp=math.nan), dict(disp_scale=0.0), dict(disp_scale=-1.0), dict(disp_scale=math.inf)):
        with pytest.raises(ValueError):
            OutputSpec(**kw)
    planes = full.empty(2, 5, 7, "cpu")
    assert [(k, tuple(v.shape), v.dtype) for k, v in planes.items()] == [("disparity", (2, 1, 5, 7), torch.uint16), ("depth", (2, 1, 5, 7), torch.uint16),
                                                                          ("uncertainties", (2, 1, 5, 7), torch.uint8)]
    st = full.struct(planes)
    assert (st.disparity.ptr, st.disparity.frame_stride, st.disparity.pitch, st.disparity.format) == (planes["disparity"].data_ptr(), 70, 14, 2)
    assert (st.uncertainty.ptr, st.uncertainty.frame_stride, st.uncertainty.pitch, st.uncertainty.format) == (planes["uncertainties"].data_ptr(), 35, 7, 3)
    assert (st.disp_scale, st.fb, st.depth_scale, st.min_disp) == (256.0, full.fb, 1000.0, 2.0 ** -8)
    assert OutputSpec(uncertainty=None).struct(OutputSpec(uncertainty=None).empty(1, 4, 4, "cpu")).uncertainty.ptr is None


def i64(t):
    return t.to(torch.int32).long() if t.dtype == torch.uint16 else t.long()


def test_reference_against_float64_away_from_ties():
    """Hand-made magnitudes with both signs; a value takes part where its float64 product lies further than 1e-3 from a tie (k + 1/2): the fp32
    product differs from the float64 one by a relative 2^-24, under 4e-3 at 65535, so away from ties both round to the same integer -- 1e-3 is
    enough below products of 16 384, and the values above that are chosen on integers."""
    from ppmstereo_amd.ppmstereo import OutputSpec
    spec = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", focal_px=721.5377, baseline=0.54, min_disp=0.5)
    g = torch.Generator().manual_seed(5)
    d = torch.cat([torch.rand(4000, generator=g) * 60.0, torch.tensor([0.6, 1.0, 3.3, 17.25, 63.999, 100.0, 191.0, 255.0, 255.99, 256.5, 300.0, 1000.0])])
    d = d * torch.where(torch.rand(d.numel(), generator=g) < 0.5, -1.0, 1.0)
    u = torch.cat([torch.rand(d.numel() - 3, generator=g), torch.tensor([0.0, 1.0, 0.5])])
    got = spec.reference(d, u)
    assert got["disparity"].dtype == torch.uint16 and got["depth"].dtype == torch.uint16 and got["uncertainties"].dtype == torch.uint8
    away = lambda p: ((p - torch.floor(p)) - 0.5).abs() > 1e-3
    D = d.double().abs()
    p = D * 256.0
    want = torch.floor(p + 0.5).clamp(max=65535)
    m = away(p)
    assert m.sum() > 3900 and torch.equal(i64(got["disparity"])[m], want.long()[m])
    fb = float(torch.tensor(721.5377, dtype=torch.float32) * torch.tensor(0.54, dtype=torch.float32))
    valid = D >= 0.5
    p = torch.where(valid, fb / D * 1000.0, torch.zeros_like(D))
    want = torch.where(valid, torch.floor(p + 0.5).clamp(max=65535), torch.zeros_like(p))
    m = ((p - torch.floor(p)) - 0.5).abs() > 0.05                # (two fp32 roundings at up to 65535 * 2^-23 each: 0.02)
    assert m.sum() > 3000 and (~valid).sum() > 10 and torch.equal(i64(got["depth"])[m], want.long()[m])
    p = u.double() * 255.0
    m = away(p)
    assert torch.equal(i64(got["uncertainties"])[m], torch.floor(p + 0.5).long()[m])
    # the float formats: magnitudes, float16 = round to nearest even of them
    f = OutputSpec(disparity="f16", depth="f32", uncertainty="f32", focal_px=721.5377, baseline=0.54, min_disp=0.5).reference(d, u)
    assert torch.equal(f["disparity"], d.abs().to(torch.float16)) and torch.equal(f["uncertainties"], u)
    assert torch.equal(f["depth"][valid], (torch.tensor(fb) / d.abs())[valid]) and torch.isposinf(f["depth"][~valid]).all()


def test_reference_ties_saturation_and_invalid_values_in_fp32():
    from ppmstereo_amd.ppmstereo import OutputSpec
    spec = OutputSpec(disparity="u16", depth="u16", uncertainty="u8", focal_px=1000.0, baseline=0.5, min_disp=0.25)
    # ties of the u16 disparity: d = k / 512 is exact in fp32 and d * 256 = k / 2 exactly: odd k round half to even
    k = torch.arange(0, 2001)
    got = i64(spec.reference(-(k.float() / 512.0), torch.zeros(k.numel()))["disparity"])
    half = k // 2
    want = torch.where(k % 2 == 0, half, torch.where(half % 2 == 0, half, half + 1))
    assert torch.equal(got, want) and want[1] == 0 and want[3] == 2 and want[5] == 2 and want[7] == 4
    nan, inf = math.nan, math.inf
    d = torch.tensor([300.0, -300.0, 255.998046875, 256.0, 0.0, -0.0, 0.125, 0.2499999, 0.25, nan, inf, 500.0, 1.0, 7.62939453125])
    u = torch.tensor([1.0, 0.0, 0.5, 0.49803921568627, 0.001, 0.002, 1.5, nan, -1.0, 0.25, 0.75, 0.1, 0.9, 0.3])
    got = spec.reference(d, u)
    assert i64(got["disparity"]).tolist() == [65535, 65535, 65535, 65535, 0, 0, 32, 64, 64, 0, 65535, 65535, 256, 1953]
    #                                         saturated: 76 800, 76 800, 65 535.5 -> 65 536, 65 536;  NaN -> 0;  7.629... * 256 = 1953.125
    # depth, fb = 500: d = 0, 0.125 and 0.2499999 lie below min_disp, NaN is invalid -> 0; d = 0.25 is valid: 2000 m -> saturates;
    # d = inf: Z = 0; d = 500: 1 m = 1000; d = 1: 500 m -> saturates; 500 / 7.62939453125 = 65.536 m -> 65536 -> 65535
    assert i64(got["depth"]).tolist() == [1667, 1667, 1953, 1953, 0, 0, 0, 0, 65535, 0, 0, 1000, 65535, 65535]
    #                                     500 / 300 * 1000 = 1666.67;  500 / 255.998 * 1000 = 1953.14
    assert i64(got["uncertainties"]).tolist() == [255, 0, 128, 127, 0, 1, 255, 0, 255, 64, 191, 26, 230, 76]
    #                                             0.5 * 255 = 127.5 -> 128 (even); 0.498... * 255 = 127.0; 1.5 saturates; NaN -> 0; |-1| = 1; 63.75; 191.25; 25.5 is no fp32 tie
    f = OutputSpec(disparity="f32", depth="f16", uncertainty=None, focal_px=1000.0, baseline=0.5, min_disp=0.25).reference(d)
    assert set(f) == {"disparity", "depth"} and f["depth"].dtype == torch.float16
    invalid = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0], dtype=torch.bool)
    assert torch.isposinf(f["depth"][invalid]).all() and torch.isfinite(f["depth"][~invalid]).all() and f["depth"][10] == 0
    assert torch.equal(torch.nan_to_num(f["disparity"], nan=-1.0), torch.nan_to_num(d.abs(), nan=-1.0)) and not torch.signbit(f["disparity"]).any()
    with pytest.raises(ValueError):
        spec.reference(d)                                         # an uncertainty plane is requested


# ---- forward_batch_test(output=...): window -> slice ------------------------------------------------------------------------------------
def test_egress_plan_hands_every_frame_to_exactly_one_window():
    """The existing host-logic tests stub nothing of forward_batch_test, so the part of its plumbing that needs no device is this function: the
    frame range each window's egress launch writes and the slice of the video it lands in (the crop is the InputPadder's geometry)."""
    from ppmstereo_amd.ppmstereo import InputPadder, egress_plan, window_plan
    assert egress_plan(window_plan(7, 4)) == [(0, 4, 0, 3, 0, 3), (2, 6, 1, 3, 3, 5), (4, 7, 1, 3, 5, 7)]
    assert egress_plan(window_plan(25, 20)) == [(0, 20, 0, 15, 0, 15), (10, 25, 5, 15, 15, 25)]
    for n, ks in ((7, 4), (25, 20), (5, 20), (40, 20), (41, 20), (33, 8), (9, 4)):
        nxt = 0
        for start, stop, keep_from, keep_to, dst_from, dst_to in egress_plan(window_plan(n, ks)):
            assert 0 <= keep_from < keep_to <= stop - start and (dst_from, dst_to) == (start + keep_from, start + keep_to) and dst_from == nxt
            nxt = dst_to
        assert nxt == n
    p = InputPadder((60, 250), divis_by=32)
    assert p.geometry() == (3, 2, 64, 256) and (p.ht, p.wd) == (60, 250)


def test_output_is_refused_where_float32_lists_or_gathers_remain():
    """The argument checks come before any device work: no GPU, no process group."""
    from ppmstereo_amd.ppmstereo import OutputSpec, PPMStereo
    m = PPMStereo.shipped(fnet=lambda x: x, cnet=lambda x: x, sst=None)
    v = torch.zeros(1, 3, 3, 64, 256)
    with pytest.raises(NotImplementedError, match="float32"):
        m.forward(v, v, iters=2, test_mode=False, output=OutputSpec())
    with pytest.raises(NotImplementedError, match="b = 1"):
        m.forward(torch.zeros(2, 3, 3, 64, 256), torch.zeros(2, 3, 3, 64, 256), iters=2, test_mode=True, output=OutputSpec())
    with pytest.raises(NotImplementedError, match="gather_kept_frames"):
        m.forward_batch_test({"stereo_video": torch.zeros(3, 2, 3, 64, 256)}, kernel_size=20, iters=2, shard_ranks=True, output=OutputSpec())
    with pytest.raises(TypeError):
        m.forward_batch_test({"stereo_video": torch.zeros(3, 2, 3, 64, 256)}, output="u16")
    with pytest.raises(ValueError):
        m.forward(v, v, iters=2, test_mode=True, crop=(0, 0, 64, 256))
