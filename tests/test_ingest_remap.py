"""CPU: rectification inside the ingest kernel.  ppms_video_ingest_u8_remap / ppms_video_ingest_yuv420_remap (raw frames of an unrectified rig
+ one fixed-point map per view -> the first-layer operands of both encoders) refuse bad arguments before touching a device (their ABI:
tests/test_ingest_doors.py); RectifyMap quantises float maps as stated, reads pointers
and pitches from views without copying, and RectifyMap.apply_u8 is the arithmetic of include/ppms.h (against ingest_util.restated_remap).
No device compute."""
import functools

import pytest
import torch

from ingest_util import EINVAL, call, lib, rand_u8, remap_view, restated_remap, yuv_view  # noqa: F401  (lib: the fixture)

NAMES = {"u8": "ppms_video_ingest_u8_remap", "yuv": "ppms_video_ingest_yuv420_remap"}


# ---- argument refusal: raw frames of 41 x 53, rectified 37 x 50 with map rows of pitch 56, two frames, padded to 64 x 64 -------------------
_map = functools.partial(remap_view, pitch=56, hs=41, ws=53)
_view = functools.partial(yuv_view, y=0x100000, u=0x200000, v=0x200001, fsy=41 * 64, fsc=21 * 64, pitch_y=64, pitch_c=64, step_c=2)      # NV12, chroma 21 x 27


def _call(lib, entry, lmap=None, rmap=None, null=(), left=0x100000, right=0x180000, frame_stride=3 * 41 * 53, lview=None, rview=None, **geometry):
    """null: indices of the maps that are NULL; geometry: ingest_util.call's."""
    from ppmstereo_amd.ppmstereo import yuv_matrix
    head = [left or None, right or None, frame_stride] if entry == "u8" else [_view(**(lview or {})), _view(**(rview or {})), yuv_matrix()]
    return call(lib, NAMES[entry], head, [_map(**(lmap or {})), _map(**(rmap or {}))], null_maps=null, **geometry)


# (what the call's message must speak of, the one thing that is wrong with the call) -- the refusals both entry points share
BAD_MAP = [("null map", dict(null=(0,))), ("null map", dict(null=(1,))),
           ("null xy or frac", dict(lmap=dict(xy=0))), ("null xy or frac", dict(rmap=dict(frac=0))),
           ("pitch", dict(lmap=dict(pitch=49))), ("pitch", dict(rmap=dict(pitch=49))),                                  # pitch < W0 = 50
           ("hs", dict(lmap=dict(hs=0), rmap=dict(hs=0))), ("ws", dict(lmap=dict(ws=32769), rmap=dict(ws=32769))),
           ("hs", dict(rmap=dict(hs=-1))), ("ws", dict(lmap=dict(ws=0))),
           ("differ", dict(rmap=dict(hs=40))), ("differ", dict(lmap=dict(ws=52))),
           ("border", dict(lmap=dict(border=2))), ("border", dict(rmap=dict(border=-1))),
           ("fill", dict(lmap=dict(fill=256))), ("fill", dict(rmap=dict(fill=-1))),
           ("reserved", dict(lmap=dict(reserved=1))), ("reserved", dict(rmap=dict(reserved=-1))),
           ("misaligned", dict(lmap=dict(xy=0x400002))), ("misaligned", dict(rmap=dict(frac=0x500001))),
           # and what video_ingest_launch refuses for every entry point
           ("skipped", dict(fnet=False, cnet=False)), ("multiples of 4", dict(H=66)), ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=-1)),
           ("positive", dict(N=0)), ("null table", dict(lut=0))]
BAD = ([(e, a, b) for e in ("u8", "yuv") for a, b in BAD_MAP if not (e == "yuv" and a == "null table")] +
       [("u8", "null source", dict(left=0)), ("u8", "null source", dict(right=0)),
        ("u8", "frame_stride", dict(frame_stride=3 * 41 * 53 - 1)),                                                    # against hs x ws, not H0 x W0
        ("yuv", "null", dict(lut=0)),
        ("yuv", "pitch_y", dict(lview=dict(pitch_y=52))), ("yuv", "pitch_c", dict(rview=dict(pitch_c=52))),             # < ws = 53, < 2 * 26 + 1
        ("yuv", "frame_stride_y", dict(lview=dict(fsy=40 * 64 + 52))), ("yuv", "frame_stride_c", dict(rview=dict(fsc=20 * 64 + 52))),
        ("yuv", "null plane", dict(lview=dict(u=0))), ("yuv", "step_c", dict(rview=dict(step_c=3))), ("yuv", "reserved", dict(lview=dict(reserved=1)))])


@pytest.mark.parametrize("entry,about,bad", BAD, ids=[e + ":" + ",".join(f"{k}={v}" for k, v in b.items()) for e, _, b in BAD])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, entry, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert _call(lib, entry, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and NAMES[entry][5:].encode() in msg and about.encode() in msg, (bad, msg)


def test_yuv_views_are_checked_against_the_source_frame(lib):
    """Views that fit the 41 x 53 source pass every view check although the rectified frame is smaller (the call is then refused by the LAST
    check made on the host, both destinations skipped); views that only fit the rectified 37 x 50 are refused."""
    assert _call(lib, "yuv", fnet=False, cnet=False) == EINVAL and b"skipped" in lib.ppms_last_error()
    small = dict(fsy=37 * 64, fsc=19 * 64)
    assert _call(lib, "yuv", lview=small, rview=small, fnet=False, cnet=False) == EINVAL and b"frame_stride" in lib.ppms_last_error()


# ---- the arithmetic, restated ------------------------------------------------------------------------------------------------------------
def random_map(H0, W0, hs, ws, seed, pitch=None):
    """xy (H0, W0, 2) int16 with x0 in [-3, ws + 2], y0 in [-3, hs + 2] and frac (H0, W0) int16 holding every one of the 1024 values (H0 W0 >= 1024),
    as views of rows of `pitch` map pixels."""
    g = torch.Generator().manual_seed(seed)
    pitch = pitch or W0
    xy, frac = torch.zeros((H0, pitch, 2), dtype=torch.int16), torch.zeros((H0, pitch), dtype=torch.int16)
    xy[:, :W0, 0] = torch.randint(-3, ws + 3, (H0, W0), generator=g).to(torch.int16)
    xy[:, :W0, 1] = torch.randint(-3, hs + 3, (H0, W0), generator=g).to(torch.int16)
    frac[:, :W0] = (torch.randperm(H0 * W0, generator=g) % 1024).to(torch.int16).reshape(H0, W0)
    return xy[:, :W0], frac[:, :W0]


# ---- RectifyMap ---------------------------------------------------------------------------------------------------------------------------
def test_from_float_against_a_float64_restatement():
    """Half-way cases round to even, negative coordinates floor (x0 = -4, fx = 22 for -3.3125), and q saturates so that x0 stays an int16."""
    from ppmstereo_amd.ppmstereo import RectifyMap
    vals = [0.0, 0.015625, 0.046875, -0.015625, -0.046875, 2.515625, 2.546875, -3.3125, -0.03125, 7.99, 31.984375, 1023.9999, -1e-9,
            32767.96875, 32767.99, 40000.0, -32768.0, -32768.02, -40000.0, float("inf"), -float("inf"), 12.3, -0.49, 100.25, 5.0]
    assert len(vals) == 25
    mx = torch.tensor(vals, dtype=torch.float32).reshape(5, 5)
    my = mx.flip(0).T.contiguous()
    m = RectifyMap.from_float(mx, my, (64, 64))

    def quantise(v):                                             # v: a Python float (float64) holding the float32 value
        if v in (float("inf"), -float("inf")):
            q = 32767 * 32 + 31 if v > 0 else -32768 * 32
        else:
            q = min(max(round(v * 32.0), -32768 * 32), 32767 * 32 + 31)       # Python's round: half to even
        return q // 32, q % 32                                   # floor and remainder

    assert m.xy.dtype == torch.int16 and tuple(m.xy.shape) == (5, 5, 2) and tuple(m.frac.shape) == (5, 5)
    for i in range(5):
        for j in range(5):
            (x0, fx), (y0, fy) = quantise(float(mx[i, j])), quantise(float(my[i, j]))
            assert (int(m.xy[i, j, 0]), int(m.xy[i, j, 1]), int(m.frac[i, j])) == (x0, y0, fx | fy << 5), (i, j)
    q = {v: quantise(float(torch.tensor(v, dtype=torch.float32))) for v in vals}
    assert q[0.015625] == (0, 0) and q[0.046875] == (0, 2) and q[-0.015625] == (0, 0) and q[-0.046875] == (-1, 30)     # 0.5 -> 0, 1.5 -> 2
    assert q[2.515625] == (2, 16) and q[2.546875] == (2, 18) and q[-3.3125] == (-4, 22)
    assert q[40000.0] == q[float("inf")] == (32767, 31) and q[-40000.0] == q[-32768.02] == (-32768, 0)
    assert (m.source_height, m.source_width, m.border, m.fill) == (64, 64, "replicate", 0)
    with pytest.raises(ValueError):
        RectifyMap.from_float(mx, my[:4], (64, 64))
    with pytest.raises(ValueError):
        RectifyMap.from_float(torch.full((2, 2), float("nan")), torch.zeros(2, 2), (64, 64))


def test_identity_copies_bytes():
    from ppmstereo_amd.ppmstereo import RectifyMap
    x = rand_u8((2, 3, 37, 50), 1)
    m = RectifyMap.identity(37, 50)
    assert (m.height, m.width, m.source_height, m.source_width, m.pitch) == (37, 50, 37, 50, 50)
    assert torch.equal(m.apply_u8(x), x)
    # constant border: the taps at x0 + 1 / y0 + 1 leave the frame in the last column / row, with weight 0 -- the constant never shows
    assert torch.equal(RectifyMap(m.xy, m.frac, (37, 50), "constant", 99).apply_u8(x), x)


def test_hand_computed_example():
    """A 2 x 2 source and four rectified pixels:
    (0,0): taps at (0,0) with fx = fy = 31: weights 1, 31, 31, 961;      R = (10 + 31*20 + 31*30 + 961*40 + 512) >> 10 = 40512 >> 10 = 39
    (0,1): x0 = 1, fx = 16: half of pixel (0,1), half of (0,2) -- outside; R = (512*20 + 512*200 + 512) >> 10 = 110 (constant 200), 20 (replicate)
    (1,0): x0 = -1, y0 = 1, frac 0: the tap is outside;                  R = 200 (constant), 30 (replicate: clamped to (1,0))
    (1,1): fx = 8, fy = 24: weights 192, 64, 576, 192;                   R = (1920 + 1280 + 17280 + 7680 + 512) >> 10 = 28672 >> 10 = 28."""
    from ppmstereo_amd.ppmstereo import RectifyMap
    src = torch.tensor([[[10, 20], [30, 40]], [[11, 21], [31, 41]], [[0, 255], [255, 0]]], dtype=torch.uint8)[None]
    xy = torch.tensor([[[0, 0], [1, 0]], [[-1, 1], [0, 0]]], dtype=torch.int16)
    frac = torch.tensor([[31 | 31 << 5, 16], [0, 8 | 24 << 5]], dtype=torch.int16)
    const = RectifyMap(xy, frac, (2, 2), "constant", 200).apply_u8(src)
    repl = RectifyMap(xy, frac, (2, 2)).apply_u8(src)
    assert const.dtype == torch.uint8 and tuple(const.shape) == (1, 3, 2, 2)
    assert const[0, 0].tolist() == [[39, 110], [200, 28]] and repl[0, 0].tolist() == [[39, 20], [30, 28]]
    assert const[0, 1].tolist() == [[40, (512 * 21 + 512 * 200 + 512) >> 10], [200, 29]] and repl[0, 1].tolist() == [[40, 21], [31, 29]]
    b11 = (64 * 255 + 576 * 255 + 512) >> 10
    assert const[0, 2].tolist() == [[(31 * 255 + 31 * 255 + 512) >> 10, (512 * 255 + 512 * 200 + 512) >> 10], [200, b11]]
    assert repl[0, 2].tolist() == [[15, 255], [255, b11]]
    for border, got in (("constant", const), ("replicate", repl)):
        assert torch.equal(got, restated_remap(src, xy, frac, border, 200))


@pytest.mark.parametrize("border,fill", [("replicate", 0), ("constant", 0), ("constant", 200)])
def test_apply_u8_against_the_restatement(border, fill):
    from ppmstereo_amd.ppmstereo import RectifyMap
    rgb = rand_u8((2, 3, 41, 53), 2)
    xy, frac = random_map(37, 50, 41, 53, 3, pitch=56)
    assert len(set(frac.reshape(-1).tolist())) == 1024
    assert int(xy[..., 0].min()) == -3 and int(xy[..., 0].max()) == 55 and int(xy[..., 1].min()) == -3 and int(xy[..., 1].max()) == 43
    m = RectifyMap(xy, frac, (41, 53), border, fill)
    got = m.apply_u8(rgb)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 37, 50) and torch.equal(got, restated_remap(rgb, xy, frac, border, fill))
    assert torch.equal(RectifyMap(xy, frac.view(torch.uint16), (41, 53), border, fill).apply_u8(rgb), got)          # uint16 frac: the same bits


def test_pitched_views_report_their_pitch_without_a_copy():
    from ppmstereo_amd.ppmstereo import RectifyMap, StereoRectifier
    xy, frac = random_map(37, 50, 41, 53, 4, pitch=56)
    m = RectifyMap(xy, frac, (41, 53), "constant", 7)
    s = m.view_struct()
    assert (s.xy, s.frac, s.pitch, s.hs, s.ws, s.border, s.fill, s.reserved) == (xy.data_ptr(), frac.data_ptr(), 56, 41, 53, 1, 7, 0)
    assert m.to("cpu") is m and (m.height, m.width) == (37, 50)
    dense = RectifyMap(xy.contiguous(), frac.contiguous(), (41, 53)).view_struct()
    assert (dense.pitch, dense.border, dense.fill) == (50, 0, 0)
    one_row = RectifyMap(xy[:1], frac[:1], (41, 53))                # a single row: its pitch is the row
    assert one_row.pitch == 50
    r = StereoRectifier(m, RectifyMap.from_float(torch.zeros(37, 50), torch.zeros(37, 50), (41, 53)))
    assert (r.height, r.width, r.source_height, r.source_width) == (37, 50, 41, 53) and r.to("cpu") is r
    assert [t.data_ptr() for t in r.tensors()] == [xy.data_ptr(), frac.data_ptr(), r.right.xy.data_ptr(), r.right.frac.data_ptr()]


def test_constructor_refusals():
    from ppmstereo_amd.ppmstereo import RectifyMap, StereoRectifier
    xy, frac = random_map(8, 12, 16, 16, 5)
    RectifyMap(xy, frac, (16, 16))
    wide_xy, wide_frac = random_map(8, 24, 16, 16, 6)
    for bad in (lambda: RectifyMap(xy.to(torch.int32), frac, (16, 16)), lambda: RectifyMap(xy, frac.float(), (16, 16)),       # dtypes
                lambda: RectifyMap(xy[..., 0], frac, (16, 16)), lambda: RectifyMap(xy, frac[:7], (16, 16)),                   # shapes
                lambda: RectifyMap(xy.permute(1, 0, 2), frac, (16, 16)), lambda: RectifyMap(xy, frac[None], (16, 16)),
                lambda: RectifyMap(wide_xy[:, ::2], wide_frac[:, ::2], (16, 16)),                                             # last dimensions not contiguous
                lambda: RectifyMap(xy, wide_frac[:, :12], (16, 16)),                                                         # two different pitches
                lambda: RectifyMap(xy, frac | 1024, (16, 16)), lambda: RectifyMap(xy, frac - 2048, (16, 16)),                # frac above 1023 (as 16 bits)
                lambda: RectifyMap(xy, frac, (0, 16)), lambda: RectifyMap(xy, frac, (16, 32769)), lambda: RectifyMap(xy, frac, 16),
                lambda: RectifyMap(xy, frac, (16, 16), border="reflect"), lambda: RectifyMap(xy, frac, (16, 16), "constant", 256)):
        with pytest.raises(ValueError):
            bad()
    m = RectifyMap(xy, frac, (16, 16))
    with pytest.raises(ValueError):
        m.apply_u8(rand_u8((1, 3, 16, 17), 7))
    with pytest.raises(ValueError):
        m.apply_u8(rand_u8((1, 3, 16, 16), 7).float())
    with pytest.raises(ValueError):
        StereoRectifier(m, RectifyMap(xy, frac, (16, 18)))        # two source sizes
    with pytest.raises(ValueError):
        StereoRectifier(m, RectifyMap.identity(16, 16))           # two rectified sizes
    with pytest.raises(TypeError):
        StereoRectifier(m, xy)


def test_model_argument_errors_come_before_any_device_work():
    from ppmstereo_amd.ppmstereo import PPMStereo, RectifyMap, StereoRectifier, YUVFrames, YUVStereoVideo
    m = PPMStereo.shipped(fnet=lambda x: x, cnet=lambda x: x, sst=None)
    ident = RectifyMap.identity(64, 256)
    r = StereoRectifier(ident, ident)
    raw = rand_u8((1, 2, 3, 64, 256), 8)
    with pytest.raises(TypeError, match="decoded bytes"):
        m.forward(raw.float(), raw.float(), iters=2, test_mode=True, rectify=r)
    with pytest.raises(TypeError, match="decoded bytes"):
        m.forward(raw, raw.float(), iters=2, test_mode=True, rectify=r)
    with pytest.raises(ValueError, match="64 x 256"):
        m.forward(raw[..., :250], raw[..., :250], iters=2, test_mode=True, rectify=r)
    with pytest.raises(TypeError, match="StereoRectifier"):
        m.forward(raw, raw, iters=2, test_mode=True, rectify=ident)
    with pytest.raises(NotImplementedError, match="b = 1"):
        m.forward(raw.expand(2, -1, -1, -1, -1), raw.expand(2, -1, -1, -1, -1), iters=2, test_mode=True, rectify=r)
    video = rand_u8((3, 2, 3, 64, 256), 9)
    with pytest.raises(TypeError, match="decoded bytes"):
        m.forward_batch_test({"stereo_video": video.float()}, iters=2, rectify=r)
    with pytest.raises(ValueError, match="64 x 256"):
        m.forward_batch_test({"stereo_video": video[..., :60, :]}, iters=2, rectify=r)
    with pytest.raises(TypeError, match="StereoRectifier"):
        m.forward_batch_test({"stereo_video": video}, iters=2, rectify=(ident, ident))
    yuv = YUVFrames.i420(rand_u8((3, 60, 256), 10), rand_u8((3, 30, 128), 11), rand_u8((3, 30, 128), 12))
    with pytest.raises(ValueError, match="64 x 256"):
        m.forward_batch_test({"stereo_video": YUVStereoVideo(yuv, yuv)}, iters=2, rectify=r)
    with pytest.raises(ValueError, match="64 x 256"):
        m.forward(yuv, yuv, iters=2, test_mode=True, rectify=r)
