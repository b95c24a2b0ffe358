"""CPU: colour out.  The 12 ppms_video_colour_* entry points and ppms_cloud_egress_colour are part of the C ABI, their ctypes bindings have the
header's argument lists, the structs keep their sizes, and every entry refuses bad arguments before touching a device -- whatever its ingest
twin refuses about sources, formats and maps with that twin's own message, and the colour arguments with one message for a door and its _remap
twin.  OutputSpec validates the new options and leaves a spec without them as it was; ``colour_bytes`` and the byte tables are the arithmetic the
issue states (literal values); ``OutputSpec.reference`` carries a colour pixel's 32 bits into the "xyzrgb" cloud unchanged, signalling-NaN
patterns included.  No device compute; every comparison is exact.  (No call in this file has nothing wrong with it: such a call would launch.)"""
import ctypes
import math

import pytest
import torch

import test_egress_cloud as CLOUD
import test_ingest_packed as PACKED
import test_ingest_raw as RAW
import test_ingest_u8 as U8
import test_ingest_yuv as YUV420
import test_ingest_yuv_deep as YUV
from colour_util import CLOUD_COLOUR, COLOUR_ARGS, ColourDoors, call_cloud_colour, random_colour_plane, said
from egress_util import CAL_700, grid_inputs, header_args, lib  # noqa: F401  (lib: the fixture)
from ingest_util import SIZE_EXPORTS, ctype_of

nan, inf = math.nan, math.inf


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [*COLOUR_ARGS, CLOUD_COLOUR])
def test_declared_exported_and_bound_as_the_header_says(lib, name):
    from ppmstereo_amd import _lib as L
    args = header_args(name)
    if name == CLOUD_COLOUR:
        assert args == header_args("ppms_cloud_egress")[:-1] + ["const ppms_egress_plane* colour", "void* stream"]
    else:
        assert args == COLOUR_ARGS[name]
    assert name in L.EXPORTS and hasattr(lib, name) and lib.ppms_version() == 4

    def ctype(arg):
        kind = arg.rsplit(" ", 1)[0]
        special = {"const ppms_egress_plane*": ctypes.POINTER(L.EgressPlane), "const ppms_cloud*": ctypes.POINTER(L.Cloud), "const float*": ctypes.c_void_p}
        return special[kind] if kind in special else ctype_of(arg)
    res, bound = L._SIGS[name]
    assert res is ctypes.c_int and bound == [ctype(a) for a in args]


def test_struct_sizes_and_format_codes_are_as_they_were(lib):
    from ppmstereo_amd import _lib as L
    assert lib.ppms_cloud_struct_size() == ctypes.sizeof(L.Cloud) == 152
    assert lib.ppms_egress_struct_size() == ctypes.sizeof(L.Egress) == 112 and lib.ppms_egress3d_struct_size() == ctypes.sizeof(L.Egress3D) == 224
    assert ctypes.sizeof(L.EgressPlane) == 32
    for name, (_, structs, sizes) in SIZE_EXPORTS.items():
        got = [ctypes.c_int() for _ in structs]
        assert getattr(lib, name)(*(ctypes.byref(x) for x in got)) == 0 and tuple(x.value for x in got) == sizes
    assert (L.FMT_F32, L.FMT_F16, L.FMT_U16, L.FMT_U8, L.FMT_RGBA8, L.FMT_BGRA8) == (0, 1, 2, 3, 4, 5)


# ---- refusals of the 12 doors -------------------------------------------------------------------------------------------------------------------
IDENTITY = dict(lmap={}, rmap={})                                                           # (maps of the frames' own 37 x 50)
# door: (the plain call, the same call through the _remap twin) -- the ingest files' own builders; with a ColourDoors for `lib` they reach the colour entry
DOOR_CALLS = {"u8": (U8._call, lambda lib, **kw: U8._call(lib, twin=True, **kw)),
              "yuv420": (YUV420._call, lambda lib, **kw: YUV420._call(lib, twin=True, **kw)),
              "yuv": (YUV._call, lambda lib, **kw: YUV._call(lib, **IDENTITY, **kw)),
              "raw": (RAW._call, lambda lib, **kw: RAW._call(lib, **IDENTITY, **kw)),
              "yuv_packed": (PACKED.yuv_call, lambda lib, **kw: PACKED.yuv_call(lib, **IDENTITY, **kw)),
              "raw_packed": (PACKED.raw_call, lambda lib, **kw: PACKED.raw_call(lib, **IDENTITY, **kw))}
# (what the message must speak of, the one thing that is wrong: changes of colour_util's TAIL / PLANE, keywords of the door's call)
COLOUR_BAD = [("table", {}, dict(lut=0)), ("null out plane", dict(null_plane=True), {}), ("null out plane", dict(ptr=0), {}),
              ("out.format", dict(format=0), {}), ("out.format", dict(format=3), {}), ("out.format", dict(format=6), {}), ("out.format", dict(format=-1), {}),
              ("out.reserved", dict(reserved=1), {}),
              ("out.pitch", dict(pitch=252), {}), ("out.pitch", dict(pitch=0), {}),                                         # 4 * w0 = 256
              ("out.frame_stride", dict(frame_stride=63 * 260 + 252), {}), ("out.frame_stride", dict(frame_stride=0), {}),  # frames that overlap
              ("multiples of the 4-byte element", dict(ptr=0x700002), {}), ("multiples of the 4-byte element", dict(pitch=258), {}),
              ("multiples of the 4-byte element", dict(frame_stride=64 * 260 + 2), {}),
              ("frame0", dict(frame0=-1), {}), ("frame0", dict(frame0=1), {}), ("frame0", dict(n_frames=3), {}),
              ("n_frames", dict(n_frames=0), {}), ("n_frames", dict(n_frames=-2), {}),
              ("h0", dict(h0=0), {}), ("w0 = -1", dict(w0=-1), {})]
COLOUR_CASES = [(door, *case) for door in DOOR_CALLS for case in COLOUR_BAD]


@pytest.mark.parametrize("door,about,changes,kw", COLOUR_CASES,
                         ids=[f"{d}:{a.replace(' ', '_')}:" + ",".join(f"{k}={v}" for k, v in {**c, **kw}.items()) for d, a, c, kw in COLOUR_CASES])
def test_colour_arguments_are_refused_with_one_message_by_a_door_and_its_twin(lib, door, about, changes, kw):
    heard = []
    for entry in DOOR_CALLS[door]:
        lib.ppms_mem_attn_splits(3, 3, 256, 1)                  # (a successful call in between: the message below is this call's)
        heard.append(said(lib, entry(ColourDoors(lib, **changes), **kw)))
    (name, text), (twin_name, twin_text) = (m.split(": ", 1) for m in heard)
    assert name == "video_colour_" + door and twin_name == name + "_remap" and text == twin_text and about in text, heard


def _door_cases():
    """The ingest files' own refusal tables, without what only the ingest launch checks (pads, H x W, the destinations) and without the calls
    that pass every check of their door ("skipped": they end at the destinations there -- here they would launch)."""
    only_ingest = {"H", "W", "pad_left", "pad_top", "fnet", "cnet"}
    tables = {"u8": [("", b) for b in U8.test_bad_arguments_return_einval_with_a_message_and_no_device.pytestmark[0].args[1]],
              "yuv420": YUV420.BAD, "yuv": YUV.BAD, "raw": RAW.BAD, "yuv_packed": PACKED.YUV_BAD, "raw_packed": PACKED.RAW_BAD}
    return [(door, bad) for door, cases in tables.items() for about, bad in cases if about not in ("skipped", "null map") and not only_ingest & set(bad)]


DOOR_CASES = _door_cases()


@pytest.mark.parametrize("door,bad", DOOR_CASES, ids=[f"{d}:{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (d, b) in enumerate(DOOR_CASES)])
def test_what_the_ingest_twin_refuses_is_refused_with_its_message(lib, door, bad):
    """Sources, formats and maps go through the ingest doors' own checks: the same code, the same message under the colour entry's name.  The plane
    of these calls has reserved = 1, which the colour launch checks behind the door: a call the door lets through ends there, not in a launch."""
    ingest = DOOR_CALLS[door][0]
    lib.ppms_mem_attn_splits(3, 3, 256, 1)
    want = said(lib, ingest(lib, **bad))
    lib.ppms_mem_attn_splits(3, 3, 256, 1)
    got = said(lib, ingest(ColourDoors(lib, reserved=1), **bad))
    assert "reserved = 1" not in got or "reserved = 1" in want, (want, got)
    if ", H = " in want:                                        # the u8 door leaves N <= 0 to the launch's check of all its sizes
        assert "must be positive" in got and got.startswith("video_colour_" + door)
    else:
        assert got == want.replace("video_ingest_", "video_colour_"), (want, got)


# ---- refusals of the coloured cloud -------------------------------------------------------------------------------------------------------------
# ppms_cloud_egress's own table where it does not depend on the record's size, and the colour call's own cases
CLOUD_SHARED = [(about, bad) for about, bad in CLOUD.BAD if not {"components", "frame_stride", "format"} & set(bad)]
CLOUD_OWN = [("components = 3", dict(components=3)), ("components = 5", dict(components=5)), ("PPMS_FMT_F32", dict(format=1)), ("format", dict(format=4)),
             ("frame_stride", dict(frame_stride=15996)),
             ("null colour plane", dict(null_colour=True)), ("null colour plane", dict(colour=dict(ptr=0))),
             ("colour.format", dict(colour=dict(format=0))), ("colour.format", dict(colour=dict(format=3))), ("colour.format", dict(colour=dict(format=6))),
             ("colour.reserved", dict(colour=dict(reserved=2))),
             ("colour.pitch", dict(colour=dict(pitch=196))),                                                                # 4 * W0 = 200
             ("colour.frame_stride", dict(colour=dict(frame_stride=36 * 204 + 196))),
             ("multiples of the 4-byte element", dict(colour=dict(ptr=0x700001))), ("multiples of the 4-byte element", dict(colour=dict(pitch=202))),
             ("multiples of the 4-byte element", dict(colour=dict(frame_stride=37 * 204 + 2)))]
CLOUD_CASES = CLOUD_SHARED + CLOUD_OWN


@pytest.mark.parametrize("about,bad", CLOUD_CASES, ids=[f"{i}:" + a.replace(" ", "_") for i, (a, _) in enumerate(CLOUD_CASES)])
def test_cloud_colour_refuses_what_cloud_egress_refuses_and_its_own(lib, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)
    msg = said(lib, call_cloud_colour(lib, **bad))
    assert msg.startswith("cloud_egress_colour: ") and about in msg, (bad, msg)


# ---- OutputSpec ---------------------------------------------------------------------------------------------------------------------------------
def test_output_spec_validation_of_the_new_options():
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd.ppmstereo import OutputSpec
    Q = OutputSpec.q_matrix(700.0, 0.25, 19.5, 11.25)
    for kw in (dict(colour="rgb8"), dict(colour=True), dict(colour="RGBA8"),
               dict(points="f32", Q=Q, points_layout="xyzrgb"), dict(points="f32", Q=Q, points_layout="xyzrgb", colour="rgba8"),
               dict(cloud="f16", Q=Q, cloud_layout="xyzrgb", colour="rgba8"), dict(cloud="f32", Q=Q, cloud_layout="xyzrgb"),
               dict(Q=Q, cloud_layout="xyzrgb", colour="bgra8"),
               dict(colour="rgba8", colour_plane=False), dict(cloud="f32", Q=Q, colour="rgba8", colour_plane=False),
               dict(cloud="f32", Q=Q, cloud_layout="xyzw", colour="rgba8", colour_plane=False), dict(colour_plane=False),
               dict(cloud="f32", Q=Q, cloud_layout="xyzrgb", colour="rgba8", colour_plane=0)):
        with pytest.raises(ValueError):
            OutputSpec(**kw)
    with pytest.raises(TypeError):                                       # the new options are keyword only
        OutputSpec("f32", None, "f32", 256.0, None, None, 1000.0, 2.0 ** -8, None, "xyz", Q, None, None, None, "xyz", False, None, "rgba8")
    # a spec without the new options is what it was
    old = OutputSpec(cloud="f16", cloud_layout="xyzw", cloud_index=True, Q=Q, points="f32", depth="u16", **CAL_700)
    assert (old.colour, old.colour_plane) == (None, True)
    assert list(old.formats()) == ["disparity", "depth", "uncertainties", "points", "cloud", "cloud_counts", "cloud_index"]
    s = OutputSpec(colour="bgra8", cloud="f32", cloud_layout="xyzrgb", cloud_index=True, cloud_capacity=20, Q=Q, points="f16", depth="u16", **CAL_700)
    assert list(s.formats().items()) == [("disparity", "f32"), ("depth", "u16"), ("uncertainties", "f32"), ("points", "f16"), ("colour", "bgra8"),
                                         ("cloud", "f32"), ("cloud_counts", "i32"), ("cloud_index", "i32")]
    assert s.cloud_components == 4 and s.points_components == 3
    planes = s.empty(2, 5, 7, "cpu")
    assert list(planes) == list(s.formats())
    assert (tuple(planes["colour"].shape), planes["colour"].dtype) == ((2, 5, 7, 4), torch.uint8)
    assert (tuple(planes["cloud"].shape), planes["cloud"].dtype) == ((2, 20, 4), torch.float32)
    assert "colour" not in s.empty(2, 5, 7, "cpu", without=("colour",))
    st = s.cloud_struct(planes, torch.empty(2, dtype=torch.int32))
    assert (st.components, st.format, st.frame_stride, st.reserved) == (4, L.FMT_F32, 20 * 16, 0)
    p = s._plane(planes["colour"], 1, s.colour)
    assert (p.ptr, p.frame_stride, p.pitch, p.format, p.reserved) == (planes["colour"].data_ptr(), 5 * 7 * 4, 7 * 4, L.FMT_BGRA8, 0)
    assert s._plane(planes["colour"], 1, "rgba8").format == L.FMT_RGBA8
    hidden = OutputSpec(colour="rgba8", colour_plane=False, cloud="f32", cloud_layout="xyzrgb", Q=Q)
    assert list(hidden.formats()) == ["disparity", "uncertainties", "cloud", "cloud_counts"] and "colour" not in hidden.empty(1, 4, 4, "cpu")
    only = OutputSpec(colour="rgba8", uncertainty=None)
    assert list(only.formats()) == ["disparity", "colour"] and not only.scene


@pytest.mark.parametrize("order", ["rgba8", "bgra8"])
def test_reference_carries_the_colour_words_into_the_cloud_bit_for_bit(order):
    """The fourth component of the "xyzrgb" cloud is ``plane.view(torch.float32)`` at the valid pixels, compared as int32: a quarter of the pixels
    hold (.., .., 0x80..0xBF, 255), the 32 bits of a signalling NaN, whose bit 22 a float operation may set."""
    from ppmstereo_amd.ppmstereo import OutputSpec
    Q = OutputSpec.q_matrix(700.0, 0.25, 19.5, 11.25)
    d, u = grid_inputs()
    plane = random_colour_plane(2, 24, 40, 5, order)
    kw = dict(Q=Q, min_disp=0.5, max_uncertainty=0.6, max_depth=40.0, cloud="f32", cloud_index=True)
    coloured = OutputSpec(colour=order, cloud_layout="xyzrgb", **kw)
    got, plain = coloured.reference(d, u, plane), OutputSpec(cloud_layout="xyzw", **kw).reference(d, u)
    assert list(got) == ["disparity", "uncertainties", "colour", "cloud", "cloud_index", "cloud_counts"] and got["colour"] is plane
    assert torch.equal(got["cloud_counts"], plain["cloud_counts"])
    words = plane.view(torch.float32).reshape(2, 24 * 40)
    snan = 0
    for f in range(2):
        count = int(got["cloud_counts"][f])
        assert 0 < count < 24 * 40 and got["cloud"][f].dtype == torch.float32 and tuple(got["cloud"][f].shape) == (count, 4)
        assert torch.equal(got["cloud_index"][f], plain["cloud_index"][f])
        assert torch.equal(got["cloud"][f][:, :3].contiguous().view(torch.int32), plain["cloud"][f][:, :3].contiguous().view(torch.int32))
        fourth = got["cloud"][f].view(torch.int32)[:, 3]
        assert torch.equal(fourth, words[f].view(torch.int32)[got["cloud_index"][f].long()])
        snan += int(((fourth >> 22) & 0x3FF == 0x3FE).sum())             # exponent all ones, sign set, bit 22 clear
    assert snan > 50
    assert "colour" not in OutputSpec(colour=order, colour_plane=False, cloud_layout="xyzrgb", **kw).reference(d, u, plane)
    for bad in (None, plane[:, :, :-1], plane.to(torch.int32), plane[..., :3]):
        with pytest.raises(ValueError):
            coloured.reference(d, u, bad)
    assert torch.equal(OutputSpec(colour=order).reference(d, u, plane)["colour"], plane)
    beside = OutputSpec(colour=order, points="f32", cloud_layout="xyzrgb", **kw)           # the keys stand in ``formats``' order
    assert list(beside.reference(d, u, plane)) == ["disparity", "uncertainties", "points", "colour", "cloud", "cloud_index", "cloud_counts"]


# ---- the colour of a pixel ----------------------------------------------------------------------------------------------------------------------
def test_colour_bytes_rounds_to_even_clamps_and_orders():
    from ppmstereo_amd.ppmstereo import colour_bytes
    values = [0.5, 1.5, 2.5, 253.5, 254.5, 0.49999997, 0.50000006, nan, -0.0, -3.0, -inf, 255.0, 255.4, 255.5, 300.0, inf, 127.5, 128.5]
    want = [0, 2, 2, 254, 254, 0, 1, 0, 0, 0, 0, 255, 255, 255, 255, 255, 128, 128]
    f = torch.tensor(values, dtype=torch.float32)
    video = torch.stack([f, f.flip(0), f.roll(5)]).reshape(1, 3, 1, len(values))          # R, G, B planes
    r, g, b = (torch.tensor(want, dtype=torch.uint8), torch.tensor(want[::-1], dtype=torch.uint8), torch.tensor(want, dtype=torch.uint8).roll(5))
    rgba, bgra = colour_bytes(video, "rgba8"), colour_bytes(video, "bgra8")
    assert rgba.dtype == torch.uint8 and tuple(rgba.shape) == (1, 1, len(values), 4)
    assert torch.equal(rgba[0, 0], torch.stack([r, g, b, torch.full_like(r, 255)], dim=-1))
    assert torch.equal(bgra[0, 0], torch.stack([b, g, r, torch.full_like(r, 255)], dim=-1))
    # read as a little-endian uint32 a "bgra8" pixel is 0xFFRRGGBB
    word = bgra.view(torch.int32)[0, 0, :, 0].to(torch.int64) & 0xFFFFFFFF
    assert word.tolist() == [0xFF000000 | int(x) << 16 | int(y) << 8 | int(z) for x, y, z in zip(r, g, b)]
    assert torch.equal(colour_bytes(video[0], "rgba8"), rgba[0])                            # any leading dimensions
    for bad in ("rgb", None, "argb8"):
        with pytest.raises(ValueError):
            colour_bytes(video, bad)
    with pytest.raises(ValueError):
        colour_bytes(video[:, :2], "rgba8")


def test_byte_tables_are_the_rounded_float_values_of_the_levels():
    """Depth 8: the level itself.  Depth 10 / 12: rint(level * 255 / (2^depth - 1)), entry for entry against integer arithmetic (no level of
    either depth lands on a tie: 2 * 255 * level is never an odd multiple of 2^depth - 1).  A tone curve: rint(tone), ties to even."""
    from ppmstereo_amd.ppmstereo import PackedRawFrames, RawFrames, YUVFrames, colour_bytes, colour_lut
    assert colour_lut("cpu", 8).tolist() == list(range(256)) and colour_lut("cpu", 8).dtype == torch.uint8
    for depth in (10, 12):
        top = (1 << depth) - 1
        assert all((2 * 255 * v) % top != 0 or (2 * 255 * v // top) % 2 == 0 for v in range(top + 1))
        assert colour_lut("cpu", depth).tolist() == [(2 * 255 * v + top) // (2 * top) for v in range(top + 1)]
        assert colour_lut("cpu", depth) is colour_lut("cpu", depth)
    with pytest.raises(ValueError):
        colour_lut("cpu", 9)
    tone = torch.rand(4096, generator=torch.Generator().manual_seed(3)).sort().values * 255.0
    tone[:6] = torch.tensor([0.0, 0.5, 1.5, 2.5, 2.5000002, 3.4999998])
    tone[-2:] = torch.tensor([254.5, 255.0])
    raw = RawFrames(torch.zeros((1, 4, 4), dtype=torch.uint16), "grbg", 12, tone=tone)
    table = raw.colour_table("cpu")
    assert table.dtype == torch.uint8 and table[:6].tolist() == [0, 0, 2, 2, 3, 3] and table[-2:].tolist() == [254, 255]
    assert torch.equal(table, torch.round(tone.double()).to(torch.uint8)) and raw[:1].colour_table("cpu") is table
    assert RawFrames(torch.zeros((1, 4, 4), dtype=torch.uint16), "grbg", 12).colour_table("cpu") is colour_lut("cpu", 12)
    assert PackedRawFrames(torch.zeros((1, 4, 5), dtype=torch.uint8), 4, "rggb", 10, tone=tone[:1024]).colour_table("cpu").tolist() == table[:1024].tolist()
    assert YUVFrames.planar(*(torch.zeros((1, 4, 4), dtype=torch.uint16),) * 3, depth=10, chroma="444").colour_table("cpu") is colour_lut("cpu", 10)
    # the table is colour_bytes of the levels' float values: what makes the kernel's bytes those of the float video
    levels = torch.arange(4096, dtype=torch.int16)
    assert torch.equal(colour_bytes(raw.levels_to_float(levels).reshape(1, 1, 4096).expand(3, 1, 4096), "rgba8")[0, :, 0], table)


def test_float_source_colour_is_colour_bytes_of_the_clamped_pixels():
    """``_FloatViews.colour``, the torch path: a rectangle that reaches over all four edges reads the replicate padding."""
    from colour_util import padded_float
    from ppmstereo_amd.ppmstereo import colour_bytes, stereo_source
    g = torch.Generator().manual_seed(9)
    video = torch.rand((3, 2, 3, 9, 11), generator=g) * 300.0 - 20.0
    source = stereo_source("test", video)
    plane = torch.full((2, 16, 16, 4), 7, dtype=torch.uint8)
    source.colour(plane, 1, 2, -3, -2, 16, 16, "bgra8")
    assert torch.equal(plane, colour_bytes(padded_float(video[1:3, 0], -3, -2, 16, 16), "bgra8"))
    with pytest.raises(ValueError):
        source.colour(plane[:, :, :, :3], 1, 2, 0, 0, 16, 16, "bgra8")
