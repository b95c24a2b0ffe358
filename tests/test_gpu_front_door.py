"""Every way into and out of PPMStereo.forward / forward_batch_test -- a float, uint8 or YUV video, on the host or the device, with or without
rectify= and output=, with this package's encoders or callables of the caller -- returns the bits of ONE canonical call.  All inputs derive
from one raw NV12 video; shapes are the smallest the model accepts (W >= 256, iters >= 2, T >= 2); every comparison is bit for bit."""
import pytest
import torch

from ppmstereo_amd.ppmstereo import OutputSpec, PPMStereo, YUVFrames, YUVStereoVideo, window_plan
from stub_encoders import StubCNet, StubFNet, frame_video
from test_gpu_block import DEV, W
from egress_util import same as same_tensor
from test_gpu_ingest_remap import raw_video, rectified_video, smooth_rectifier
from ingest_util import model, same  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu
SPEC = dict(disparity="u16", uncertainty="u8")
RAW, RECT = (70, 262), (60, 250)                 # raw frames -> rectified 60 x 250 -> padded 64 x 256 with odd pads on both axes


def on_device(video):
    return video.to(DEV)


def on_host(video):
    return video


def quantised(ref):
    return OutputSpec(**SPEC).reference(ref["disparity"], ref["uncertainties"])


def same_planes(out, want):
    return set(out) == set(want) == {"disparity", "uncertainties"} and all(same_tensor(out[k], want[k]) for k in want)


def check_doors(run, doors, n):
    """doors: (name, video, rectifier or None, canonical result).  Each, from the host and from the device, without and with output=."""
    for name, video, rectify, ref in doors:
        kw = {} if rectify is None else {"rectify": rectify}
        for place in (on_host, on_device):
            out = run(place(video), **kw)
            assert tuple(out["disparity"].shape) == (n, 1, *ref["disparity"].shape[-2:]) and not out["disparity"].is_cuda, (name, place.__name__)
            assert same(out, ref), (name, place.__name__)
            q = run(place(video), output=OutputSpec(**SPEC), **kw)
            assert q["disparity"].dtype == torch.uint16 and q["uncertainties"].dtype == torch.uint8, (name, place.__name__)
            assert same_planes(q, quantised(ref)), (name, place.__name__, "output=")


def doors_of(yuv, rgb, rect, r, canonical, raw_canonical):
    return [("float", rect.float(), None, canonical), ("uint8", rect, None, canonical), ("uint8 + rectify", rgb, r, canonical),
            ("yuv", yuv, None, raw_canonical), ("yuv + rectify", yuv, r, canonical)]


def test_package_encoders_single_window(model):
    r = smooth_rectifier(*RECT, *RAW, 11)
    yuv, rgb = raw_video(3, *RAW, 111)
    rect = rectified_video(rgb, r)
    assert tuple(rect.shape) == (3, 2, 3, *RECT)
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=2, **kw)
    canonical = run(rect)
    assert same(canonical, run(rect)), "the uint8 path itself is not repeatable: nothing can be said about the other doors"
    assert torch.isfinite(canonical["disparity"]).all() and (quantised(canonical)["disparity"].to(torch.int32) > 0).any()
    raw_canonical = run(rgb)                     # a YUV video without rectify= is its RGB bytes at the raw size
    assert tuple(raw_canonical["disparity"].shape) == (3, 1, *RAW)
    check_doors(run, doors_of(yuv, rgb, rect, r, canonical, raw_canonical), 3)


def test_package_encoders_three_windows(model):
    """7 frames, kernel_size 4: three windows through the ClipPipeline."""
    assert len(window_plan(7, 4)) == 3
    r = smooth_rectifier(*RECT, *RAW, 12, "constant", 128)
    yuv, rgb = raw_video(7, *RAW, 112)
    rect = rectified_video(rgb, r)
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=2, **kw)
    canonical = run(rect)
    assert same(canonical, run(rect)), "the uint8 path itself is not repeatable: nothing can be said about the other doors"
    check_doors(run, doors_of(yuv, rgb, rect, r, canonical, run(rgb)), 7)


def test_rectify_with_diagnostics(model):
    r = smooth_rectifier(*RECT, *RAW, 13)
    yuv, rgb = raw_video(3, *RAW, 113)
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=20, iters=2, diagnostics=True, **kw)
    canonical = run(rectified_video(rgb, r))
    assert canonical["attn_redo"] and canonical["attn_redo"]["1/4"]["calls"] == 2
    for video in (rgb, yuv, on_device(yuv)):
        out = run(video, rectify=r)
        assert out["attn_redo"] == canonical["attn_redo"] and same(out, canonical)
    q = run(yuv, rectify=r, output=OutputSpec(**SPEC))
    assert q.pop("attn_redo") == canonical["attn_redo"] and same_planes(q, quantised(canonical))


def test_forward_directly(model):
    """YUV frames with output= and frames=; raw uint8 frames with rectify=, output= and crop=: the reference of the plain call's tensors."""
    yuv, rgb = raw_video(3, *RAW, 114)
    spec = OutputSpec(**SPEC)
    host = lambda planes: {k: v.cpu() for k, v in planes.items()}
    # the top left 64 x 256 of every plane: strided views of the raw surfaces
    left, right = (YUVFrames(v.y[:, :64, :256], v.u[:, :32, :128], v.v[:, :32, :128]).to(DEV) for v in (yuv.left, yuv.right))
    i1, i2 = (rgb[None, :, k, :, :64, :256].to(DEV) for k in (0, 1))
    rd, ru = model.forward(i1, i2, iters=2, test_mode=True)
    d, u = model.forward(left, right, iters=2, test_mode=True)
    assert tuple(d.shape) == (1, 3, 1, 64, 256) and torch.equal(d, rd) and torch.equal(u, ru)
    out = model.forward(left, right, iters=2, test_mode=True, output=spec, frames=(1, 3))
    torch.cuda.synchronize()
    assert tuple(out["disparity"].shape) == (1, 2, 1, 64, 256) and out["disparity"].is_cuda
    assert same_planes(host(out), spec.reference(rd[:, 1:3].cpu(), ru[:, 1:3].cpu()))
    r = smooth_rectifier(64, 256, *RAW, 14)
    raw1, raw2 = rgb[None, :, 0].to(DEV), rgb[None, :, 1].to(DEV)
    rd, ru = model.forward(raw1, raw2, iters=2, test_mode=True, rectify=r)
    rect = rectified_video(rgb, r).to(DEV)
    pd, pu = model.forward(rect[None, :, 0], rect[None, :, 1], iters=2, test_mode=True)
    assert tuple(rd.shape) == (1, 3, 1, 64, 256) and torch.equal(rd, pd) and torch.equal(ru, pu)
    for a, b in ((raw1, raw2), (yuv.left.to(DEV), yuv.right.to(DEV))):
        out = model.forward(a, b, iters=2, test_mode=True, rectify=r, output=spec, crop=(5, 3, 40, 200))
        torch.cuda.synchronize()
        assert tuple(out["disparity"].shape) == (1, 3, 1, 40, 200)
        assert same_planes(host(out), spec.reference(rd[..., 3:43, 5:205].cpu(), ru[..., 3:43, 5:205].cpu()))


@pytest.fixture(scope="module")
def stub_model():
    return PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(W).to(DEV).eval()


def grey_video(rgb):
    """Full-range grey frames (Y, 128, 128): the YUVStereoVideo whose RGB bytes are the constant frames of ``rgb`` (N, 2, 3, H, W)."""
    n, h, w = rgb.shape[0], rgb.shape[-2], rgb.shape[-1]
    chroma = lambda: torch.full((n, (h + 1) // 2, (w + 1) // 2), 128, dtype=torch.uint8)
    return YUVStereoVideo(*(YUVFrames.i420(rgb[:, k, 0].clone(), chroma(), chroma(), full_range=True) for k in (0, 1)))


@pytest.mark.parametrize("n,kernel_size", [(3, 20), (7, 4)])
def test_callers_encoders(stub_model, n, kernel_size):
    """Encoder callables of the caller (stub_encoders.py, keyed on a frame's grey level; a constant frame stays that constant under a
    replicate-border remap): every door takes the float path and returns the stub model's own canonical bits."""
    r = smooth_rectifier(*RECT, *RAW, 15)
    raw, rect = frame_video(n, *RAW).to(torch.uint8), frame_video(n, *RECT).to(torch.uint8)
    assert torch.equal(rectified_video(raw, r), rect)
    run = lambda v, **kw: stub_model.forward_batch_test({"stereo_video": v}, kernel_size=kernel_size, iters=2, **kw)
    canonical = run(rect)
    assert same(canonical, run(rect)), "the stub model itself is not repeatable"
    assert torch.isfinite(canonical["disparity"]).all()
    check_doors(run, [("float", rect.float(), None, canonical), ("uint8", rect, None, canonical), ("uint8 + rectify", raw, r, canonical),
                      ("yuv", grey_video(rect), None, canonical), ("yuv + rectify", grey_video(raw), r, canonical)], n)


def test_callers_encoders_forward_directly(stub_model):
    spec = OutputSpec(**SPEC)
    host = lambda planes: {k: v.cpu() for k, v in planes.items()}
    r = smooth_rectifier(64, 256, *RAW, 16)
    raw, rect = frame_video(3, *RAW).to(torch.uint8), frame_video(3, 64, 256).to(torch.uint8).to(DEV)
    rd, ru = stub_model.forward(rect[None, :, 0], rect[None, :, 1], iters=2, test_mode=True)
    grey = on_device(grey_video(rect.cpu()))
    out = stub_model.forward(grey.left, grey.right, iters=2, test_mode=True, output=spec, frames=(1, 3))
    torch.cuda.synchronize()
    assert same_planes(host(out), spec.reference(rd[:, 1:3].cpu(), ru[:, 1:3].cpu()))
    want = spec.reference(rd[..., 3:43, 5:205].cpu(), ru[..., 3:43, 5:205].cpu())
    graw = on_device(grey_video(raw))
    for a, b in ((raw[None, :, 0].to(DEV), raw[None, :, 1].to(DEV)), (graw.left, graw.right)):
        out = stub_model.forward(a, b, iters=2, test_mode=True, rectify=r, output=spec, crop=(5, 3, 40, 200))
        torch.cuda.synchronize()
        assert same_planes(host(out), want)
