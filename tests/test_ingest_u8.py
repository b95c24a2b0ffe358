"""CPU: ppms_video_ingest_u8 (uint8 video -> the first-layer operands of both encoders) refuses bad arguments before touching a
device (its ABI: tests/test_ingest_doors.py), and the pad geometry handed to it is InputPadder's.  No compute."""
import pytest
import torch

from ingest_util import EINVAL, call, lib, remap_view  # noqa: F401  (lib: the fixture)

NAME = "ppms_video_ingest_u8"


def _call(lib, left=0x1000, right=0x2000, stride=3 * 37 * 50, twin=False, **geometry):
    """Two frames of 37 x 50 padded to 64 x 64 (ingest_util.call).  twin: through the _remap twin, with maps whose source frame is H0 x W0."""
    maps = [remap_view(hs=geometry.get("H0", 37), ws=geometry.get("W0", 50))] * 2 if twin else ()
    return call(lib, NAME + "_remap" * twin, [left or None, right or None, stride], maps, **geometry)


@pytest.mark.parametrize("bad", [dict(left=0, right=0, lut=0), dict(left=0), dict(right=0), dict(lut=0),      # NULL pointers
                                 dict(H=66), dict(W=62, pad_left=6),                                        # H % 4, W % 4
                                 dict(pad_left=15), dict(pad_top=28), dict(pad_left=-1), dict(pad_top=-1),  # pad + source > padded size, negative pads
                                 dict(N=0), dict(stride=3 * 37 * 50 - 1), dict(fnet=False, cnet=False)])
def test_bad_arguments_return_einval_with_a_message_and_no_device(lib, bad):
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert _call(lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and b"video_ingest_u8" in msg, (bad, msg)


def test_destination_views_follow_img_s2d_contract(lib):
    from ppmstereo_amd import _lib as L
    ok = L.SP(0x10000, 0x20000, 32, 32)
    for view in (L.SP(0x10000, None, 32, 32), L.SP(0x10000, 0x20000, 32, 8), L.SP(0x10000, 0x20000, 36, 32), L.SP(0x10008, 0x20000, 32, 32)):
        assert lib.ppms_video_ingest_u8(0x1000, 0x2000, 3 * 32 * 32, 1, 32, 32, 0, 0, 32, 32, 0x3000, view, L.SP(None, None, 0, 0), None) == EINVAL
        assert b"destination" in lib.ppms_last_error()
    small = L.SP(0x10000, 0x20000, 40, 40)                      # the k = 4 operand holds 48 values
    assert lib.ppms_video_ingest_u8(0x1000, 0x2000, 3 * 32 * 32, 1, 32, 32, 0, 0, 32, 32, 0x3000, ok, small, None) == EINVAL


@pytest.mark.parametrize("h0,w0", [(37, 50), (60, 250), (64, 256), (33, 65)])
def test_pad_geometry_is_input_padders(h0, w0):
    from ppmstereo_amd.ppmstereo import InputPadder
    padder = InputPadder((1, 3, h0, w0), divis_by=32)
    pad_left, pad_top, H, W = padder.geometry()
    x = torch.arange(h0 * w0, dtype=torch.float32).reshape(1, 1, h0, w0)
    (padded,) = padder.pad(x)
    assert tuple(padded.shape[-2:]) == (H, W) and H % 32 == 0 and W % 32 == 0 and H - h0 < 32 and W - w0 < 32
    assert [pad_left, W - w0 - pad_left, pad_top, H - h0 - pad_top] == padder._pad
    # the source pixel (0, 0) sits at (pad_top, pad_left); everything in front of it replicates it; unpad is the inverse crop
    assert torch.equal(padded[0, 0, :pad_top + 1, :pad_left + 1], torch.zeros(pad_top + 1, pad_left + 1))
    assert padded[0, 0, pad_top, pad_left + 1] == 1.0 and padded[0, 0, pad_top + 1, pad_left] == float(w0)
    assert torch.equal(padder.unpad(padded), x)
    # the clamped source coordinate the kernel uses is replicate padding
    ys = (torch.arange(H) - pad_top).clamp(0, h0 - 1)
    xs = (torch.arange(W) - pad_left).clamp(0, w0 - 1)
    assert torch.equal(padded[0, 0], x[0, 0][ys][:, xs])


def test_public_interface():
    import inspect

    from ppmstereo_amd.cnet import Feature, _CnetEngine
    from ppmstereo_amd.encoder import BasicEncoder, _FnetEngine
    for enc, eng in ((BasicEncoder, _FnetEngine), (Feature, _CnetEngine)):
        assert list(inspect.signature(enc.plan).parameters)[1:] == ["N", "H", "W", "device"]
        assert callable(eng.s0_view) and callable(eng.run_filled) and list(inspect.signature(eng.run).parameters)[1:] == ["img"]
