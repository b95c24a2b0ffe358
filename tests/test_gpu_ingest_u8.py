"""GPU: the uint8 front door.  ppms_video_ingest_u8 against the float path's own op chain on the same device -- u8.float(), InputPadder.pad,
2 * (x / 255.0) - 1.0, torch.cat, ppms_img_s2d -- and PPMStereo.forward / forward_batch_test on a uint8 video against the same calls on its
.float().  Every comparison is bit-exact (both bf16 planes as int16; torch.equal on the model outputs): the kernel looks the normalised
value of a byte up in a table the float path's expression built, and shares split_bf16 with ppms_img_s2d."""
import pytest
import torch

from ppmstereo_amd import _lib as L
from ingest_util import DEV, bits, float_path_operands, ingest, model, patterned, rand_u8, same  # noqa: F401  (model: the fixture)
from test_gpu_block import W

pytestmark = pytest.mark.gpu
NONE_SP = L.SP(None, None, 0, 0)


def test_byte_table_is_the_float_paths_expression():
    from ppmstereo_amd.ppmstereo import byte_lut
    lut = byte_lut(DEV)
    x = torch.arange(256, dtype=torch.uint8, device=DEV).reshape(1, 1, 16, 16).float()
    assert lut.dtype == torch.float32 and torch.equal(lut, (2 * (x / 255.0) - 1.0).reshape(-1)) and byte_lut(DEV) is lut


def test_kernel_window_layout_with_odd_padding():
    """One (T, 2, 3, 37, 50) block -> 64 x 64: left / right pad 7 / 7, top / bottom 13 / 14, rows of 50 bytes (no alignment), both borders."""
    from ppmstereo_amd.ppmstereo import InputPadder
    win = rand_u8((2, 2, 3, 37, 50), 11).to(DEV)
    padder = InputPadder((37, 50), divis_by=32)
    assert padder._pad == [7, 7, 13, 14]
    pad_left, pad_top, H, Wd = padder.geometry()
    ef, ec, He, We = float_path_operands(win[:, 0], win[:, 1], padder._pad)
    assert (H, Wd) == (He, We) == (64, 64)
    f, c = patterned(4 * 32 * 32, 32), patterned(2 * 16 * 16, 64)
    ingest(win[:, 0].data_ptr(), win[:, 1].data_ptr(), 6 * 37 * 50, 2, 37, 50, pad_left, pad_top, H, Wd, f.view(), c.view())
    assert win[:, 1].data_ptr() == win.data_ptr() + 3 * 37 * 50
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))
    assert not bits(f)[:, :, 12:].any() and not bits(c)[:, :, 48:].any() and bits(f)[:, :, :12].any()       # tail channels zeroed


def test_kernel_separate_tensors_and_skipped_destinations():
    """Two (3, 3, 32, 64) tensors, frame_stride 3 * 32 * 64, no padding; a destination with hi == NULL is skipped and stays as it was."""
    left, right = rand_u8((3, 3, 32, 64), 12).to(DEV), rand_u8((3, 3, 32, 64), 13).to(DEV)
    ef, ec, H, Wd = float_path_operands(left, right, [0, 0, 0, 0])
    for skip in ("cnet", "fnet"):
        f, c = patterned(6 * 16 * 32, 32), patterned(3 * 8 * 16, 64)
        before_f, before_c = bits(f).clone(), bits(c).clone()
        fv, cv = f.view(), c.view()
        if skip == "cnet":
            cv.hi = None                                         # (lo, ld, c stay set: hi == NULL alone must be enough to skip)
        else:
            fv.hi = None
        ingest(left.data_ptr(), right.data_ptr(), 3 * 32 * 64, 3, 32, 64, 0, 0, H, Wd, fv, cv)
        if skip == "cnet":
            assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), before_c)
        else:
            assert torch.equal(bits(c), bits(ec)) and torch.equal(bits(f), before_f)


def test_kernel_block_straddling_both_destinations():
    """36 x 36 from 33 x 35: the k = 2 part is 2592 threads, so one 256-thread block serves the end of one destination and the start of the other."""
    left, right = rand_u8((1, 3, 33, 35), 14).to(DEV), rand_u8((1, 3, 33, 35), 15).to(DEV)
    ef, ec, H, Wd = float_path_operands(left, right, [1, 0, 2, 1])
    assert (H, Wd) == (36, 36) and (2 * 18 * 18 * 4) % 256
    f, c = patterned(2 * 18 * 18, 32), patterned(9 * 9, 64)
    ingest(left.data_ptr(), right.data_ptr(), 3 * 33 * 35, 1, 33, 35, 1, 2, H, Wd, f.view(), c.view())
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))


def test_kernel_frame_stride_past_2_to_31():
    """Frame 1 of each view lies more than 2^31 bytes behind frame 0 (an odd stride): the source offset is 64-bit arithmetic."""
    H0, W0, stride = 8, 12, (1 << 31) + 4097
    frames = rand_u8((2, 2, 3, H0, W0), 16).to(DEV)               # [frame][view]
    buf = torch.empty(stride + 2 * 3 * H0 * W0, dtype=torch.uint8, device=DEV)
    n = 3 * H0 * W0
    for t in range(2):
        buf[t * stride:t * stride + 2 * n] = frames[t].reshape(-1)
    ef, ec, H, Wd = float_path_operands(frames[:, 0], frames[:, 1], [0, 0, 0, 0])
    f, c = patterned(4 * 4 * 6, 32), patterned(2 * 2 * 3, 64)
    ingest(buf.data_ptr(), buf.data_ptr() + n, stride, 2, H0, W0, 0, 0, H, Wd, f.view(), c.view())
    assert torch.equal(bits(f), bits(ef)) and torch.equal(bits(c), bits(ec))


def test_model_single_window(model):
    """(3, 2, 3, 60, 250) -> 64 x 256 (the smallest width the pyramid accepts), one window: the uint8 video gives the float video's bits,
    from the host and from the device."""
    video = rand_u8((3, 2, 3, 60, 250), 21)
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    ref, ref2 = run(video.float()), run(video.float())
    assert same(ref, ref2), "the float path itself is not repeatable: nothing can be said about the uint8 path"
    out = run(video)
    assert tuple(out["disparity"].shape) == (3, 1, 60, 250) and not out["disparity"].is_cuda and out["disparity"].dtype == torch.float32
    assert torch.isfinite(out["disparity"]).all() and same(out, ref)
    assert same(run(video.to(DEV)), ref)


def test_model_several_windows_take_the_clip_pipeline(model):
    from ppmstereo_amd.ppmstereo import window_plan
    video = rand_u8((7, 2, 3, 60, 250), 22)
    assert len(window_plan(7, 4)) > 1
    run = lambda v: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2)
    ref = run(video.float())
    out = run(video)
    assert tuple(out["disparity"].shape) == (7, 1, 60, 250) and same(out, ref)


def test_model_forward_directly(model):
    i1, i2 = rand_u8((1, 3, 3, 64, 256), 23).to(DEV), rand_u8((1, 3, 3, 64, 256), 24).to(DEV)
    d, u = model.forward(i1, i2, iters=4, test_mode=True)
    rd, ru = model.forward(i1.float(), i2.float(), iters=4, test_mode=True)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.equal(d, rd) and torch.equal(u, ru)
    with pytest.raises(TypeError):
        model.forward(i1, i2.float(), iters=4, test_mode=True)
    with pytest.raises(TypeError):
        model.forward(i1.float(), i2, iters=4, test_mode=True)
    # b > 1 and every prediction (test_mode=False) behave as for float input
    j1, j2 = rand_u8((2, 2, 3, 64, 256), 25).to(DEV), rand_u8((2, 2, 3, 64, 256), 26).to(DEV)
    p, q = model.forward(j1, j2, iters=2, test_mode=False)
    rp, rq = model.forward(j1.float(), j2.float(), iters=2, test_mode=False)
    assert tuple(p.shape) == (4, 2, 2, 1, 64, 256) and torch.equal(p, rp) and torch.equal(q, rq)


def test_user_supplied_encoders_get_float_images():
    """Encoder callables of the caller (the stand-ins of stub_encoders.py): the uint8 video is converted on the device and takes the float path."""
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet, frame_video
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()
    video = frame_video(7, 60, 250)
    run = lambda v: m.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=4)
    assert same(run(video.to(torch.uint8)), run(video))
    v = frame_video(3, 64, 256).to(DEV)
    d, u = m.forward(v[None, :, 0].to(torch.uint8), v[None, :, 1].to(torch.uint8), iters=4, test_mode=True)
    rd, ru = m.forward(v[None, :, 0], v[None, :, 1], iters=4, test_mode=True)
    assert torch.equal(d, rd) and torch.equal(u, ru)
