"""CPU: the raw-sensor front door (Bayer mosaics and monochrome planes of 8, 10 or 12 bits).  ppms_video_ingest_raw and its _remap twin refuse bad
arguments before touching a device (their ABI: tests/test_ingest_doors.py);
RawFrames.to_rgb is the demosaic, black level and white balance the header states (against a per-pixel restatement in plain Python), RawFrames reads
byte strides from views without copying, and stereo_source dispatches raw frames without a device.  No device compute."""
import ctypes
import functools
import itertools

import pytest
import torch

from ingest_util import EINVAL, call_twin, lib, rand_u8, rand_u16, raw_view  # noqa: F401  (lib: the fixture)

NAME, REMAP = "ppms_video_ingest_raw", "ppms_video_ingest_raw_remap"
PATTERNS = ["rggb", "bggr", "grbg", "gbrg", "mono"]
COLOURS = PATTERNS[:4]
FORMATS = [(8, "lsb"), (10, "lsb"), (10, "msb"), (12, "lsb"), (12, "msb")]            # (depth, align)


# ---- argument refusal: BayerRG10 frames (bits at the top) of 37 x 50 in surfaces of pitch 128 bytes, two frames, padded to 64 x 64 ---------------
_view = functools.partial(raw_view, data=0x100000, fs=37 * 128, pitch=128)


def _call(lib, left=None, right=None, fmt=None, null=(), lmap=None, rmap=None, null_rmap=False, **geometry):
    """geometry: ingest_util.call's.  lmap / rmap (dicts): the _remap twin."""
    from ppmstereo_amd import _lib as L
    f = dict(sample_bytes=2, depth=10, lsb=6, pattern=0, black=64, gain=(1536, 1024, 1300), shift=10, reserved=(0, 0, 0))
    f.update(fmt or {})
    head = [_view(**(left or {})), _view(**(right or {})),
            L.RawFormat(f["sample_bytes"], f["depth"], f["lsb"], f["pattern"], f["black"], f["gain"], f["shift"], f["reserved"])]
    return call_twin(lib, NAME, head, null, lmap, rmap, null_rmap, **geometry)


BYTES = dict(sample_bytes=1, depth=8, lsb=0)                          # (with the 16-bit views' strides, which are large enough for bytes too)
DEEP12 = dict(depth=12, lsb=4)
OFF = dict(fnet=False, cnet=False)                                    # (a call that passes every raw check gets as far as the destinations)
# (what the call's message must speak of, the one thing that is wrong with the call)
BAD = [  # null pointers
       ("null", dict(null=(0,))), ("null", dict(null=(1,))), ("null", dict(null=(2,))), ("null", dict(lut=0)),
       ("null data", dict(left=dict(data=0))), ("null data", dict(right=dict(data=0))),
       # non-zero reserved
       ("reserved", dict(left=dict(reserved=1))), ("reserved", dict(right=dict(reserved=-1))),
       ("reserved", dict(fmt=dict(reserved=(1, 0, 0)))), ("reserved", dict(fmt=dict(reserved=(0, 0, -1)))),
       # sample_bytes / depth / lsb outside the table
       ("sample_bytes", dict(fmt=dict(sample_bytes=0))), ("sample_bytes", dict(fmt=dict(sample_bytes=3))), ("sample_bytes", dict(fmt=dict(sample_bytes=4))),
       ("depth", dict(fmt=dict(sample_bytes=1, depth=10, lsb=0))), ("depth", dict(fmt=dict(depth=8, lsb=0))), ("depth", dict(fmt=dict(depth=11, lsb=0))),
       ("depth", dict(fmt=dict(depth=14, lsb=0))), ("depth", dict(fmt=dict(depth=16, lsb=0))), ("depth", dict(fmt=dict(sample_bytes=1, depth=12, lsb=0))),
       ("lsb", dict(fmt=dict(lsb=1))), ("lsb", dict(fmt=dict(lsb=4))), ("lsb", dict(fmt=dict(depth=12, lsb=6))), ("lsb", dict(fmt=dict(lsb=-6))),
       ("lsb", dict(fmt=dict(sample_bytes=1, depth=8, lsb=8))),
       # the mosaic, the black level, the white balance
       ("pattern", dict(fmt=dict(pattern=-1))), ("pattern", dict(fmt=dict(pattern=5))),
       ("black", dict(fmt=dict(black=-1))), ("black", dict(fmt=dict(black=1024))), ("black", dict(fmt=dict(BYTES, black=256))),
       ("black", dict(fmt=dict(DEEP12, black=4096))),
       ("gain", dict(fmt=dict(gain=(-1, 1024, 1024)))), ("gain", dict(fmt=dict(gain=(1024, 16 << 10, 1024)))),
       ("gain", dict(fmt=dict(gain=(1024, 1024, 16 << 10)))), ("gain", dict(fmt=dict(gain=(16 << 4, 16, 16), shift=4))),
       ("shift", dict(fmt=dict(shift=3))), ("shift", dict(fmt=dict(shift=15))), ("shift", dict(fmt=dict(shift=-1))),
       # 16-bit samples at odd addresses
       ("odd", dict(left=dict(data=0x100001))), ("odd", dict(right=dict(pitch=129))), ("odd", dict(left=dict(fs=37 * 128 + 1))),
       # rows and frames that overlap
       ("pitch", dict(left=dict(pitch=98))), ("pitch", dict(right=dict(pitch=98))), ("pitch", dict(fmt=BYTES, left=dict(pitch=49))),
       ("frame_stride", dict(left=dict(fs=36 * 128 + 98))), ("frame_stride", dict(right=dict(fs=0))),
       ("frame_stride", dict(fmt=BYTES, right=dict(fs=36 * 128 + 49))),
       # a colour pattern on a frame without neighbours
       ("2 x 2", dict(H0=1)), ("2 x 2", dict(W0=1)), ("2 x 2", dict(fmt=dict(pattern=3), H0=1, W0=1)),
       # sizes, pads and destinations: video_ingest_launch's checks
       ("skipped", OFF), ("multiples of 4", dict(H=66)), ("multiples of 4", dict(W=62, pad_left=6)),
       ("do not fit", dict(pad_left=15)), ("do not fit", dict(pad_top=28)), ("do not fit", dict(pad_left=-1)), ("do not fit", dict(pad_top=-1)),
       ("positive", dict(N=0)), ("positive", dict(H0=0)), ("positive", dict(W0=-2)),
       # (what is legal passes the raw checks: a single frame needs no frame stride, a monochrome frame no neighbours, the bounds themselves)
       ("skipped", dict(OFF, N=1, left=dict(fs=0), right=dict(fs=2))), ("skipped", dict(OFF, fmt=dict(pattern=4), H0=1, W0=1)),
       ("skipped", dict(OFF, fmt=dict(black=1023, gain=(0, (16 << 10) - 1, 1)))), ("skipped", dict(OFF, fmt=dict(shift=14, gain=((16 << 14) - 1,) * 3))),
       ("skipped", dict(OFF, fmt=dict(shift=4, gain=(255, 0, 16)))), ("skipped", dict(OFF, H0=2, W0=2)),
       ("skipped", dict(OFF, fmt=dict(BYTES, pattern=2, black=255), left=dict(data=0x100001, pitch=51, fs=37 * 51))),
       # the _remap twin: what the existing _remap calls refuse, a fill that is no level, and the raw checks against hs x ws
       ("null map", dict(null_rmap=True)), ("null xy", dict(lmap=dict(xy=0))), ("fill", dict(lmap=dict(fill=1024))), ("fill", dict(rmap=dict(fill=-1))),
       ("fill", dict(fmt=BYTES, lmap=dict(fill=256))), ("fill", dict(fmt=DEEP12, rmap=dict(fill=4096))),
       ("pitch =", dict(lmap=dict(pitch=49))), ("border", dict(rmap=dict(border=2))), ("hs, ws", dict(rmap=dict(hs=36))),
       ("source frame", dict(lmap=dict(hs=0), rmap=dict(hs=0))), ("reserved", dict(rmap=dict(reserved=1))), ("misaligned", dict(lmap=dict(frac=0x500001))),
       ("depth", dict(lmap=dict(), fmt=dict(depth=9))), ("lsb", dict(rmap=dict(), fmt=dict(lsb=2))), ("odd", dict(lmap=dict(), left=dict(pitch=127))),
       ("pattern", dict(lmap=dict(), fmt=dict(pattern=7))), ("null", dict(rmap=dict(), null=(2,))),
       ("pitch", dict(lmap=dict(ws=65), rmap=dict(ws=65))),                                                  # 130 bytes a row
       ("frame_stride", dict(lmap=dict(hs=38), rmap=dict(hs=38))), ("2 x 2", dict(lmap=dict(hs=1), rmap=dict(hs=1))),
       ("skipped", dict(OFF, lmap=dict(fill=1023))), ("skipped", dict(OFF, fmt=DEEP12, rmap=dict(fill=4095))),
       ("skipped", dict(OFF, lmap=dict(hs=30, ws=64), rmap=dict(hs=30, ws=64)))]


@pytest.mark.parametrize("about,bad", BAD, ids=[f"{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (_, b) in enumerate(BAD)])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, about, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert _call(lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_raw" in msg and about.encode() in msg, (bad, msg)
    assert (b"video_ingest_raw_remap" in msg) == ("lmap" in bad or "rmap" in bad or "null_rmap" in bad), msg


def test_destination_views_follow_img_s2d_contract(lib):
    from ppmstereo_amd import _lib as L
    v, f = _view(fs=32 * 128), L.RawFormat(2, 12, 0, 1, 0, (1024, 1024, 1024), 10, (0, 0, 0))
    call = lambda fd, cd: lib.ppms_video_ingest_raw(ctypes.byref(v), ctypes.byref(v), ctypes.byref(f), 1, 32, 32, 0, 0, 32, 32, 0x3000, fd, cd, None)
    for view in (L.SP(0x10000, None, 32, 32), L.SP(0x10000, 0x20000, 32, 8), L.SP(0x10000, 0x20000, 36, 32), L.SP(0x10008, 0x20000, 32, 32)):
        assert call(view, L.SP(None, None, 0, 0)) == EINVAL
        assert b"destination" in lib.ppms_last_error() and b"video_ingest_raw" in lib.ppms_last_error()
    assert call(L.SP(0x10000, 0x20000, 32, 32), L.SP(0x10000, 0x20000, 40, 40)) == EINVAL      # the k = 4 operand holds 48 values


# ---- the arithmetic, restated pixel by pixel ---------------------------------------------------------------------------------------------------
TILES = {"rggb": "RGGB", "bggr": "BGGR", "grbg": "GRBG", "gbrg": "GBRG"}


def reflect(t, n):
    """A neighbour coordinate outside 0 .. n - 1, reflected without repeating the edge."""
    if t < 0:
        t = -t
    if t > n - 1:
        t = 2 * (n - 1) - t
    assert 0 <= t <= n - 1
    return t


def restated_levels(samples, pattern, depth, black=0, gains=(1024, 1024, 1024), shift=10):
    """samples: nested lists [N][hs][ws] of Python integers (the samples themselves, already cut out of their words) -> [N][3][hs][ws] levels by the
    header's rules, one pixel and one channel at a time."""
    top = 2 ** depth - 1
    out = []
    for frame in samples:
        hs, ws = len(frame), len(frame[0])
        s = lambda y, x: frame[reflect(y, hs)][reflect(x, ws)]
        planes = [[[0] * ws for _ in range(hs)] for _ in range(3)]
        for y, x, c in itertools.product(range(hs), range(ws), range(3)):
            want = "RGB"[c]
            if pattern == "mono":
                v = frame[y][x]
            else:
                tile = TILES[pattern]
                colour = lambda yy, xx: tile[(yy % 2) * 2 + (xx % 2)]
                k = colour(y, x)
                if want == k:
                    v = frame[y][x]
                elif k in "RB" and want == "G":
                    assert {colour(y - 1, x), colour(y + 1, x), colour(y, x - 1), colour(y, x + 1)} == {"G"}
                    v = (s(y - 1, x) + s(y + 1, x) + s(y, x - 1) + s(y, x + 1) + 2) // 4
                elif k in "RB":
                    assert {colour(y + dy, x + dx) for dy in (-1, 1) for dx in (-1, 1)} == {want}
                    v = (s(y - 1, x - 1) + s(y - 1, x + 1) + s(y + 1, x - 1) + s(y + 1, x + 1) + 2) // 4
                elif colour(y, x + 1) == want:
                    assert colour(y, x - 1) == want
                    v = (s(y, x - 1) + s(y, x + 1) + 1) // 2
                else:
                    assert colour(y - 1, x) == colour(y + 1, x) == want
                    v = (s(y - 1, x) + s(y + 1, x) + 1) // 2
            planes[c][y][x] = min(top, max(0, ((v - black) * gains[c] + 2 ** (shift - 1)) // 2 ** shift))       # // floors, as >> does
        out.append(planes)
    return out


def raw_words(shape, seed, depth, align):
    """(the words a driver would leave, the samples in them): random samples of `depth` bits, with garbage in the unused bits of 16-bit words."""
    if depth == 8:
        data = rand_u8(shape, seed)
        return data, data.to(torch.int64)
    low = 16 - depth
    samples = rand_u16(shape, seed, 1 << depth).to(torch.int64)
    junk = rand_u16(shape, seed + 1000, 1 << low).to(torch.int64)
    words = (samples << low) | junk if align == "msb" else samples | (junk << depth)
    assert bool(junk.any()) and bool((words != (samples << low if align == "msb" else samples)).any())
    return words.to(torch.int32).to(torch.uint16), samples


@pytest.mark.parametrize("depth,align", FORMATS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_to_rgb_against_the_per_pixel_restatement(pattern, depth, align):
    from ppmstereo_amd.ppmstereo import RawFrames
    top = 2 ** depth - 1
    for i, (hs, ws) in enumerate([(2, 2), (2, 3), (3, 2), (5, 6), (7, 5)]):
        words, samples = raw_words((2, hs, ws), 10 * i + depth, depth, align)
        for black, gains in ((0, (1.0, 1.0, 1.0)), (top // 16, (1.71, 1.0, 2.33))):
            f = RawFrames(words, pattern, depth, align, black, gains)
            q = tuple(round(g * 1024) for g in gains)
            assert f.gain_q == q and tuple(f.format_struct().gain) == q and f.format_struct().shift == 10
            got = f.to_rgb()
            assert got.dtype == (torch.uint8 if depth == 8 else torch.int16) and tuple(got.shape) == (2, 3, hs, ws)
            assert got.tolist() == restated_levels(samples.tolist(), pattern, depth, black, q)


@pytest.mark.parametrize("pattern", COLOURS)
def test_a_solid_colour_demosaics_to_itself_at_every_pixel(pattern):
    """Every R site a, every G site b, every B site c -> (a, b, c) everywhere, borders and corners included: a reflection that repeated the edge,
    or a clamp, would mix another colour into the border pixels of some size."""
    from ppmstereo_amd.ppmstereo import RawFrames
    tile = TILES[pattern]
    for (hs, ws), depth in itertools.product([(2, 2), (2, 3), (3, 2), (3, 3), (4, 4), (4, 5), (5, 4), (6, 7), (7, 7), (8, 6)], (8, 12)):
        a, b, c = (200, 17, 96) if depth == 8 else (4000, 5, 1234)
        value = {"R": a, "G": b, "B": c}
        plane = torch.tensor([[value[tile[(y % 2) * 2 + (x % 2)]] for x in range(ws)] for y in range(hs)], dtype=torch.int32)
        data = plane.to(torch.uint8 if depth == 8 else torch.uint16)[None]
        rgb = RawFrames(data, pattern, depth).to_rgb()
        want = torch.tensor([a, b, c], dtype=rgb.dtype).reshape(1, 3, 1, 1).expand(1, 3, hs, ws)
        assert torch.equal(rgb, want), (pattern, hs, ws, depth)


@pytest.mark.parametrize("depth,align", FORMATS)
def test_black_level_and_gains_in_python_integers(depth, align):
    """A monochrome plane holding every level once (v is the sample): level = clamp(floor((v - black) g / 2^shift + 1 / 2)), as exact rationals."""
    from fractions import Fraction
    from ppmstereo_amd.ppmstereo import RawFrames
    top, n = 2 ** depth - 1, 2 ** depth
    lsb = 16 - depth if (depth > 8 and align == "msb") else 0
    v = torch.arange(n, dtype=torch.int32)
    data = (v << lsb).to(torch.uint8 if depth == 8 else torch.uint16).reshape(1, n // 16, 16)
    for black, gains in ((0, (1.0, 1.0, 1.0)), (n // 16, (0.0, 0.5, 15.99)), (top, (2.0, 1.0, 1.0)), (n // 8, (1.0009765625, 3.7, 1.2))):
        f = RawFrames(data, "mono", depth, align, black, gains)
        got = f.to_rgb().reshape(3, n).tolist()
        for c, g in enumerate(f.gain_q):
            assert g == round(gains[c] * 1024)
            want = [min(top, max(0, ((x - black) * Fraction(g, 1024) + Fraction(1, 2)).__floor__())) for x in range(n)]
            assert got[c] == want, (black, gains, c)
            assert all(w == 0 for w in want[:black + 1])                   # at and below the black level: 0
        if gains[2] > 15:
            assert got[2][-1] == top and got[2].count(top) > n // 2        # a saturating gain: the top level
    assert torch.equal(RawFrames(data, "mono", depth, align).to_rgb().reshape(3, n).long(), v.long().expand(3, n))      # unit gains: the identity


def test_to_float_and_the_tone_curve():
    from ppmstereo_amd.ppmstereo import RawFrames
    words, _ = raw_words((2, 5, 8), 71, 10, "lsb")
    f = RawFrames(words, "grbg", 10)
    levels = f.to_rgb()
    assert f.to_float().dtype == torch.float32 and torch.equal(f.to_float(), levels.float() * (255.0 / 1023))
    b = RawFrames(rand_u8((2, 5, 6), 72), "bggr")
    assert b.to_rgb().dtype == torch.uint8 and torch.equal(b.to_float(), b.to_rgb().float())
    tone = 255.0 * (torch.arange(1024, dtype=torch.float64) / 1023) ** (1 / 2.2)
    g = RawFrames(words, "grbg", 10, tone=tone)
    assert g.tone.dtype == torch.float32 and torch.equal(g.to_rgb(), levels)             # the curve comes behind the levels
    assert torch.equal(g.to_float(), tone.float()[levels.long()]) and g.to_float().dtype == torch.float32
    assert g[1:].tone is g.tone and g.split_side_by_side()[1].tone is g.tone and torch.equal(g[1:].to_float(), g.to_float()[1:])
    for bad in (tone[:-1], tone[:256], tone.reshape(32, 32), tone + 0.5, tone - 0.5, torch.full((1024,), float("nan")), torch.arange(1024), tone.tolist()):
        with pytest.raises(ValueError):
            RawFrames(words, "grbg", 10, tone=bad)
    with pytest.raises(ValueError):
        RawFrames(rand_u8((2, 5, 6), 73), "mono", tone=tone)               # 1024 values for 256 levels


# ---- RawFrames on host tensors ---------------------------------------------------------------------------------------------------------------
def test_byte_strides_are_read_from_views():
    from ppmstereo_amd.ppmstereo import RawFrames
    surface = rand_u16((3, 37, 64), 74)                         # a pitched 16-bit surface: 50 of 64 words per row are picture
    f = RawFrames(surface[:, :, :50], "gbrg", 12, "msb", black=256, gains=(1.5, 1.0, 2.0))
    s, fmt = f.view_struct(), f.format_struct()
    assert (f.n, f.height, f.width, len(f), f.depth, f.align, f.pattern, f.sample_bytes, f.device) == (3, 37, 50, 3, 12, "msb", "gbrg", 2, surface.device)
    assert (s.data, s.pitch, s.frame_stride, s.reserved) == (surface.data_ptr(), 128, 37 * 128, 0)
    assert (fmt.sample_bytes, fmt.depth, fmt.lsb, fmt.pattern, fmt.black, list(fmt.gain), fmt.shift, list(fmt.reserved)) == \
        (2, 12, 4, 3, 256, [1536, 1024, 2048], 10, [0, 0, 0])
    assert [RawFrames(surface[:, :, :50], p, 10).format_struct().pattern for p in PATTERNS] == [0, 1, 2, 3, 4]
    assert RawFrames(surface[:, :, :50], "rggb", 10).lsb == 0 and RawFrames(surface[:, :, :50], "rggb", 10, "msb").lsb == 6
    win = f[1:3]                                                # a slice of frames: the same surface, one frame further
    assert len(win) == 2 and win.view_struct().data == surface.data_ptr() + 37 * 128 and win.view_struct().frame_stride == 37 * 128
    assert (win.pattern, win.depth, win.align, win.black, win.gains) == ("gbrg", 12, "msb", 256, (1.5, 1.0, 2.0))
    assert torch.equal(win.to_rgb(), f.to_rgb()[1:3])
    one = f[2:]                                                 # a single frame: a plane's size stands in for the stride, in bytes
    assert (one.n, one.frame_stride, one.pitch) == (1, 2 * (36 * 64 + 50), 128)
    with pytest.raises(TypeError):
        f[1]
    bytes_ = rand_u8((2, 9, 33), 75)
    m = RawFrames(bytes_[:, 1:8, 3:30], "mono")                 # odd offsets and odd pitches are fine for bytes
    assert (m.view_struct().data, m.pitch, m.frame_stride, m.sample_bytes, m.lsb) == (bytes_.data_ptr() + 33 + 3, 33, 9 * 33, 1, 0)
    assert RawFrames(bytes_, "rggb", align="msb").lsb == 0        # (align is ignored at depth 8)
    assert f.to("cpu") is f                                     # (nothing to copy: the frames are there)


def test_packed_frames_split_without_a_copy():
    from ppmstereo_amd.ppmstereo import RawFrames, RawStereoVideo
    packed = rand_u16((3, 32, 128), 76, 1024)
    p = RawFrames(packed, "grbg", 10, black=64)
    left, right = p.split_side_by_side()
    l, r = left.view_struct(), right.view_struct()
    assert (l.data, r.data - l.data) == (packed.data_ptr(), 128) and (r.pitch, r.frame_stride, l.pitch, l.frame_stride) == (256, 32 * 256, 256, 32 * 256)
    for half in (left, right):
        assert (half.height, half.width, half.pattern, half.depth, half.black) == (32, 64, "grbg", 10, 64)
    video = RawStereoVideo(left, right)
    assert (len(video), video.height, video.width, video.depth) == (3, 32, 64, 10)
    win = video[1:3]
    assert len(win) == 2 and win.right.view_struct().data == packed.data_ptr() + 32 * 256 + 128 and torch.equal(win.right.to_rgb(), right.to_rgb()[1:3])
    assert video.to("cpu").left is left
    # away from the seam, a half's interior pixels are the packed frame's (at the seam each half reflects where the packed frame reads on)
    full = p.to_rgb()
    assert torch.equal(left.to_rgb()[..., :63], full[..., :63]) and torch.equal(right.to_rgb()[..., 1:], full[..., 65:])
    top, bottom = p.split_top_bottom()
    assert bottom.view_struct().data - top.view_struct().data == 16 * 256 and (bottom.height, bottom.width) == (16, 128)
    assert torch.equal(bottom.to_rgb()[:, :, 1:], full[:, :, 17:])
    # a half that starts on an odd column or row would have another pattern: refused; a monochrome frame only needs an even packed size
    odd_w, odd_h = rand_u8((1, 6, 10), 77), rand_u8((1, 10, 6), 78)
    for pattern in COLOURS:
        with pytest.raises(ValueError):
            RawFrames(odd_w, pattern).split_side_by_side()
        with pytest.raises(ValueError):
            RawFrames(odd_h, pattern).split_top_bottom()
        even = RawFrames(rand_u8((1, 8, 12), 89), pattern)
        assert even.split_side_by_side()[1].width == 6 and even.split_top_bottom()[1].height == 4
    a, b = RawFrames(odd_w, "mono").split_side_by_side()
    assert (a.width, b.width, b.view_struct().data - a.view_struct().data) == (5, 5, 5)
    assert RawFrames(odd_h, "mono").split_top_bottom()[1].height == 5
    for pattern in PATTERNS:
        with pytest.raises(ValueError):
            RawFrames(rand_u8((1, 6, 9), 79), pattern).split_side_by_side()       # an odd packed width
        with pytest.raises(ValueError):
            RawFrames(rand_u8((1, 9, 6), 80), pattern).split_top_bottom()


def test_what_is_no_raw_frame_raises():
    from ppmstereo_amd.ppmstereo import RawFrames
    d8, d16 = rand_u8((2, 8, 12), 81), rand_u16((2, 8, 12), 82)
    RawFrames(d8), RawFrames(d16, depth=10), RawFrames(d16, "mono", 12, "msb", 4095, (0.0, 15.99, 1.0))
    RawFrames(d8[:, :1, :1], "mono")
    wide = rand_u16((2, 8, 24), 83)
    for bad in (lambda: RawFrames(d16), lambda: RawFrames(d8, depth=10), lambda: RawFrames(d16.to(torch.int16), depth=10),
                lambda: RawFrames(d8.float()), lambda: RawFrames(d8[0]), lambda: RawFrames(d8.tolist()), lambda: RawFrames(d8[:0]),
                lambda: RawFrames(d8, "rgbg"), lambda: RawFrames(d8, "RGGB"), lambda: RawFrames(d16, depth=14), lambda: RawFrames(d16, depth=16),
                lambda: RawFrames(d16, depth=10, align="left"),
                lambda: RawFrames(wide[:, :, ::2], depth=10),                                     # samples two words apart
                lambda: RawFrames(d8.as_strided((2, 8, 12), (96, 6, 1))),                         # rows that overlap
                lambda: RawFrames(d8.as_strided((2, 8, 12), (40, 12, 1))),                        # frames that overlap
                lambda: RawFrames(d8[:, :1], "rggb"), lambda: RawFrames(d8[:, :, :1], "gbrg"),    # a colour pattern without neighbours
                lambda: RawFrames(d8, black=-1), lambda: RawFrames(d8, black=256), lambda: RawFrames(d16, depth=10, black=1024),
                lambda: RawFrames(d8, black=1.5),
                lambda: RawFrames(d8, gains=(1.0, 1.0)), lambda: RawFrames(d8, gains=(-0.1, 1.0, 1.0)), lambda: RawFrames(d8, gains=(1.0, 16.0, 1.0)),
                lambda: RawFrames(d8, gains=(1.0, 1.0, float("nan"))), lambda: RawFrames(d8, gains=1.0), lambda: RawFrames(d8, gains=("a", 1, 1))):
        with pytest.raises(ValueError):
            bad()


# ---- the front doors' argument checks ----------------------------------------------------------------------------------------------------
def test_mismatched_pairs_are_no_stereo_video():
    from ppmstereo_amd.ppmstereo import RawFrames, RawStereoVideo
    d = rand_u16((2, 8, 12), 84, 1024)
    tone = torch.linspace(0, 255, 1024)
    base = RawFrames(d, "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone)
    same = RawFrames(d.clone(), "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone.clone())          # an equal curve in another tensor
    assert len(RawStereoVideo(base, same)) == 2
    others = [RawFrames(d, "bggr", 10, "lsb", 64, (1.5, 1.0, 2.0), tone), RawFrames(d, "mono", 10, "lsb", 64, (1.5, 1.0, 2.0), tone),
              RawFrames(d, "rggb", 12, "lsb", 64, (1.5, 1.0, 2.0), torch.linspace(0, 255, 4096)), RawFrames(d, "rggb", 10, "msb", 64, (1.5, 1.0, 2.0), tone),
              RawFrames(d, "rggb", 10, "lsb", 65, (1.5, 1.0, 2.0), tone), RawFrames(d, "rggb", 10, "lsb", 64, (1.5, 1.0, 2.001), tone),
              RawFrames(d, "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0)), RawFrames(d, "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone.flip(0)),
              RawFrames(d[:1], "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone), RawFrames(d[:, :6], "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone),
              RawFrames(d[:, :, :10], "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0), tone),
              RawFrames(rand_u8((2, 8, 12), 85), "rggb", 8, "lsb", 64, (1.5, 1.0, 2.0))]
    for other in others:
        with pytest.raises(ValueError):
            RawStereoVideo(base, other)
        with pytest.raises(ValueError):
            RawStereoVideo(other, base)
    with pytest.raises(TypeError):
        RawStereoVideo(base, d)
    assert len(RawStereoVideo(others[6], RawFrames(d, "rggb", 10, "lsb", 64, (1.5, 1.0, 2.0)))) == 2       # no curve on either side


def test_stereo_source_checks_without_a_device():
    from ppmstereo_amd.ppmstereo import RawFrames, RawStereoVideo, RectifyMap, StereoRectifier, YUVFrames
    from ppmstereo_amd.video import _ByteSource, stereo_source
    d = rand_u16((2, 32, 64), 86, 1024)
    tone = 255.0 * (torch.arange(1024, dtype=torch.float32) / 1023) ** 0.45
    left, right = RawFrames(d, "gbrg", 10, black=64, gains=(1.8, 1.0, 1.4), tone=tone), RawFrames(d.flip(0), "gbrg", 10, black=64, gains=(1.8, 1.0, 1.4), tone=tone)
    src = stereo_source("PPMStereo.forward", left, right)
    assert isinstance(src, _ByteSource) and (src.n, src.b, src.size, src.depth, src._entry) == (2, 1, (32, 64), 10, "ppms_video_ingest_raw")
    frames = src._frames()
    assert len(frames) == 3 and frames[0].data == d.data_ptr() and frames[2].pattern == 3 and src._maps == ()
    assert src._planes()[0] is left.data and src.held()[1] is right.data
    video = RawStereoVideo(left, right)
    assert stereo_source("forward_batch_test", video)._entry == "ppms_video_ingest_raw"
    assert stereo_source("forward_batch_test", video[:1]).n == 1
    with pytest.raises(ValueError):                                                          # no stereo pair
        stereo_source("PPMStereo.forward", left, RawFrames(d, "grbg", 10, black=64, gains=(1.8, 1.0, 1.4), tone=tone))
    y, c = rand_u8((2, 32, 64), 87), rand_u8((2, 16, 32), 88)
    for a, b in ((left, d), (d, right), (left, YUVFrames.i420(y, c, c.clone())), (YUVFrames.i420(y, c, c.clone()), right), (left, None)):
        with pytest.raises(TypeError):
            stereo_source("PPMStereo.forward", a, b)
    with pytest.raises(TypeError):
        stereo_source("PPMStereo.forward", left, right, rectify="maps")
    ident = RectifyMap(RectifyMap.identity(32, 64).xy, RectifyMap.identity(32, 64).frac, (32, 64), "constant", 255)
    rect = stereo_source("forward_batch_test", video, rectify=StereoRectifier(ident, ident))
    assert rect._entry == "ppms_video_ingest_raw_remap" and [m.fill for m in rect._maps] == [1023, 1023] and rect.size == (32, 64)
    small = StereoRectifier(RectifyMap(ident.xy[:20, :30], ident.frac[:20, :30], (32, 64)), RectifyMap(ident.xy[:20, :30], ident.frac[:20, :30], (32, 64)))
    assert stereo_source("forward_batch_test", video, rectify=small).size == (20, 30)        # the results' size is the rectified one
    with pytest.raises(ValueError):                                                          # frames of another size than the maps' source
        stereo_source("forward_batch_test", video, rectify=StereoRectifier(RectifyMap.identity(30, 64), RectifyMap.identity(30, 64)))
    # the path of other encoder callables: to_float(), and with maps the tone curve behind the blend
    fl, fr = src.float_views()
    assert torch.equal(fl, left.to_float()) and torch.equal(fr, right.to_float()) and fl.dtype == torch.float32 and tuple(fr.shape) == (2, 3, 32, 64)
    l2, _ = rect.float_views()
    assert torch.equal(l2, tone[ident.apply_levels(left.to_rgb(), 10).long()])
    plain = stereo_source("PPMStereo.forward", RawFrames(d, "mono", 10), RawFrames(d.clone(), "mono", 10))
    assert torch.equal(plain.float_views()[0], (d.to(torch.int32)[:, None].expand(2, 3, 32, 64)).float() * (255.0 / 1023))
