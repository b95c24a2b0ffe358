"""GPU: the correlation pyramid build (corr.hip: the line-resident kernel and the general one), the convex upsamplings and the tap
gather-sum (loop_ops.hip), the bilinear resize and the four tiled transposes (glue_ops.hip), each called through the C ABI and compared
with the plain float64 reference of tests/kernel_refs.py.

Tolerances (kernel_refs.py states the rule; none comes from the code under test): (a) exact for the transposes and the accum side of the
gather-sum; (c) for the pyramid levels, both upsamplings and the resize 8 x the max error of the same operation in plain fp32 torch on
the CPU on the same input; the gather-sum's out within (ntap + 1) 2^-24 (|bias| + sum |terms|) per element, the first-order worst case of
any-order fp32 summation.  Every output sits in a buffer pre-filled with a sentinel (1.0) -- the pyramid levels with NaN, a sentinel gap
after each --, padding columns of the inputs hold junk, frames beyond the temporal halo NaN; whatever lies outside what a kernel owns still
holds its fill after the launch."""
import ctypes

import pytest
import torch

import kernel_refs as R
from kernel_refs import f32_in, f32_out, planes_are, report, sp_in_junk, sp_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ids = lambda c: "x".join(map(str, c)).replace(" ", "")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ correlation pyramid
@pytest.mark.parametrize("case", list(R.CORR_CASES))
def test_corr_build(lib, case):
    """ppms_corr_build, every level against float64 (kind c).  The five levels lie in one NaN-filled buffer (a NaN that survives is an
    element nobody wrote: an infinite error) with a sentinel gap after each level, which must survive; level 0 is 16-byte and level 1
    8-byte aligned, so that the aligned cases run the line-resident kernel (32 / 64 / 128 wide, C / 16 = 2, 3, 1, 4 stages per x2 block)
    and the others the general one."""
    L, lb = lib, lib.load()
    B, C, H, W, misaligned = R.CORR_CASES[case]
    feats = []
    for f in R.corr_inputs(case):
        buf = torch.full((f.numel() + 8,), R.JUNK, device=DEV)
        v = buf[int(misaligned):int(misaligned) + f.numel()].view_as(f)
        v.copy_(f)
        assert v.data_ptr() % 16 == (4 if misaligned else 0)
        feats.append(v)
    rows = B * H * W
    sizes = [rows * (W >> l) for l in range(5)]
    store = torch.full((sum(sizes) + sum(R.CORR_GAPS),), NAN, device=DEV)
    levels, gaps, off = [], [], 0
    for n, g in zip(sizes, R.CORR_GAPS):
        levels.append(store[off:off + n])
        gaps.append(store[off + n:off + n + g])
        gaps[-1].fill_(R.SENTINEL)
        off += n + g
    if W % 4 == 0:
        assert levels[0].data_ptr() % 16 == 0 and levels[1].data_ptr() % 8 == 0
    ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in levels])
    L.check(lb.ppms_corr_build(feats[0].data_ptr(), feats[1].data_ptr(), ptrs, B, C, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.corr_check(case, [t.view(rows, W >> l) for l, t in enumerate(levels)]))
    assert all(bool((g == R.SENTINEL).all()) for g in gaps), "the gap after a level must not be written"


# ------------------------------------------------------------------------------------------------ convex upsampling
def _convex_launch(L, dim, case, data):
    """-> the (T, 2, 4 H, 4 W) output.  The flow buffer holds NaN around what the launch may read: CONVEX_HALO frames on either side for
    the 3-D kernel, of which the t_halo next to the own frames are filled; a row and a pixel for the 2-D one"""
    lb = L.load()
    T, H, W = case[:3]
    ld, HW = case[-1], H * W
    flow, mask, th = R.convex_inputs(dim, case, data)
    before = R.CONVEX_HALO * HW if dim == 3 else W + 1
    fd = torch.full((2 * before + T * HW, 2), NAN, device=DEV)
    fd[before - th * HW:before + (T + th) * HW] = flow.reshape(-1, 2).to(DEV)
    md = f32_in(mask.reshape(T * HW, -1), ld)
    n = T * 2 * 16 * HW
    out = f32_out(n)
    if dim == 3:
        L.check(lb.ppms_convex_upsample_3d(fd[before:].data_ptr(), md.data_ptr(), ld, out.data_ptr(), T, H, W, th, L.stream_ptr()))
    else:
        L.check(lb.ppms_convex_upsample(fd[before:].data_ptr(), md.data_ptr(), ld, out.data_ptr(), T, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (out[n:] == R.SENTINEL).all()
    return out[:n].view(T, 2, 4 * H, 4 * W)


@pytest.mark.parametrize("data", R.CONVEX_DATA)
@pytest.mark.parametrize("case", R.CONVEX2D_CASES, ids=ids)
def test_convex_upsample(lib, case, data):
    """ppms_convex_upsample at the leading dimensions the engine passes (mask_ch, 144 and wider) against float64 (kind c): N(0, 1) logits,
    logits whose exp overflows fp32 without the max, and a flow of magnitude ~60"""
    report(R.convex_check(2, case, data, _convex_launch(lib, 2, case, data)))


@pytest.mark.parametrize("data", R.CONVEX_DATA)
@pytest.mark.parametrize("case", R.CONVEX3D_CASES, ids=ids)
def test_convex_upsample_3d(lib, case, data):
    """ppms_convex_upsample_3d without a halo (the unsharded engine; T = 1: two thirds of the taps outside), with one and with two halo
    frames, mask_ld 432 and wider"""
    report(R.convex_check(3, case, data, _convex_launch(lib, 3, case, data)))


# ------------------------------------------------------------------------------------------------ tap gather-sum
@pytest.mark.parametrize("case", R.TGS_CASES, ids=lambda c: ids((c[0], *c[1], *c[2:])))
def test_tap_gather_sum(lib, case):
    """ppms_tap_gather_sum on y given directly (independent of any conv): out within the any-order fp32 summation bound of float64, accum
    += out exactly; the padding columns of out and accum keep the sentinel.  Frames of y beyond t_halo hold NaN, its columns from
    ntap * cout on junk."""
    L, lb = lib, lib.load()
    cout, k3, T, H, W, th, y_ld, out_ld, accum_ld = case
    HW, P = H * W, T * H * W
    y, bias, acc0 = R.tgs_inputs(case)
    yd = torch.full(((T + 2 * R.TGS_HALO) * HW, y_ld), NAN, device=DEV)
    own = yd[(R.TGS_HALO - th) * HW:(R.TGS_HALO + T + th) * HW]
    own.fill_(R.JUNK)
    own[:, :y.shape[1]] = y.to(DEV)
    bd = bias.to(DEV)
    out = f32_out(P * out_ld)
    accum = None
    if accum_ld is not None:
        accum = f32_out(P * accum_ld)
        accum[:P * accum_ld].view(P, accum_ld)[:, :cout] = acc0.to(DEV)
    L.check(lb.ppms_tap_gather_sum(yd[R.TGS_HALO * HW:].data_ptr(), y_ld, bd.data_ptr(), out.data_ptr(), out_ld,
                                   None if accum is None else accum.data_ptr(), accum_ld or 0, cout, *k3, T, H, W, th, L.stream_ptr()))
    torch.cuda.synchronize()
    o = out[:P * out_ld].view(P, out_ld)
    a = None if accum is None else accum[:P * accum_ld].view(P, accum_ld)
    report(R.tgs_check(case, o[:, :cout], None if a is None else a[:, :cout]))
    assert (o[:, cout:] == R.SENTINEL).all() and (out[P * out_ld:] == R.SENTINEL).all(), "the padding columns of out must not be written"
    if a is not None:
        assert (a[:, cout:] == R.SENTINEL).all() and (accum[P * accum_ld:] == R.SENTINEL).all(), "the padding columns of accum must not be written"


# ------------------------------------------------------------------------------------------------ bilinear resize
@pytest.mark.parametrize("mul", R.BILINEAR_MUL)
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=ids)
def test_bilinear(lib, case, align, mul):
    """ppms_bilinear against float64 F.interpolate times mul (kind c): up, down, the identity, one output pixel (the zero scale of
    align_corners), a 1 x 1 source"""
    L, lb = lib, lib.load()
    N, C, H, W, OH, OW = case
    xd = R.bilinear_input(case).to(DEV)
    n = N * C * OH * OW
    out = f32_out(n)
    L.check(lb.ppms_bilinear(xd.data_ptr(), out.data_ptr(), N, C, H, W, OH, OW, align, mul, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.bilinear_check(case, bool(align), mul, out[:n].view(N, C, OH, OW)))
    assert (out[n:] == R.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ tiled transposes
def _sp_round_trip(L, BT, C, HW, channels, c0):
    """ppms_nchw_to_sp into channels [c0, c0 + C) of a sentinel-filled SP tensor, then ppms_sp_to_nchw out of a junk-filled one"""
    lb = L.load()
    x = R.transpose_input(BT, C, HW)
    P, want = BT * HW, R.to_channel_last(x)
    xd = x.to(DEV)
    t = sp_out(L, P, channels)
    L.check(lb.ppms_nchw_to_sp(xd.data_ptr(), t.view(c0, C), BT, C, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    d = t.own().cpu()
    hi, lo = R.sp_split(want)
    ck = R.Check(f"nchw_to_sp {(BT, C, HW, channels, c0)}").exact("hi", d[0, :, c0:c0 + C], hi).exact("lo", d[1, :, c0:c0 + C], lo)
    assert planes_are(t, 0, c0, R.SENTINEL) and planes_are(t, c0 + C, channels, R.SENTINEL), "the channels around the view must not be written"
    s = sp_in_junk(L, R.sp_round(want), channels, c0)
    n = BT * C * HW
    back = f32_out(n)
    L.check(lb.ppms_sp_to_nchw(s.view(c0, C), back.data_ptr(), BT, C, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    report(ck.exact("sp_to_nchw", back[:n].view(BT, C, HW), R.sp_round(x)))
    assert (back[n:] == R.SENTINEL).all()


@pytest.mark.parametrize("case", R.TRANSPOSE_CASES, ids=ids)
def test_nchw_sp_transposes(lib, case):
    """all-distinct values over 2^-20 .. 2^20, so that any permutation or frame-stride slip shows: the SP destination holds sp_split(x) in
    both planes bit for bit, the way back gives sp_round(x); the engine's own calls (C = 2, 144, 432, 256) among the shapes"""
    BT, C, HW, ld = case
    _sp_round_trip(lib, BT, C, HW, ld, 0)


def test_nchw_sp_transposes_on_a_channel_view(lib):
    """a 33-channel view at channel offset 8 of a 48-channel SP tensor"""
    BT, C, HW, channels, c0 = R.TRANSPOSE_SP_VIEW
    _sp_round_trip(lib, BT, C, HW, channels, c0)


@pytest.mark.parametrize("case", R.TRANSPOSE_CASES, ids=ids)
def test_nchw_to_nhwc(lib, case):
    L, lb = lib, lib.load()
    BT, C, HW, ld = case
    x = R.transpose_input(BT, C, HW)
    xd = x.to(DEV)
    P = BT * HW
    dst = f32_out(P * ld)
    L.check(lb.ppms_nchw_to_nhwc(xd.data_ptr(), dst.data_ptr(), ld, BT, C, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    d = dst[:P * ld].view(P, ld)
    report(R.Check(f"nchw_to_nhwc {case}").exact("dst", d[:, :C], R.to_channel_last(x)))
    assert (d[:, C:] == R.SENTINEL).all() and (dst[P * ld:] == R.SENTINEL).all(), "the padding columns must not be written"


@pytest.mark.parametrize("case", R.TRANSPOSE_CASES + R.TRANSPOSE_F32_SRC_EXTRA, ids=ids)
def test_nhwc_to_nchw(lib, case):
    L, lb = lib, lib.load()
    BT, C, HW, ld = case
    x = R.transpose_input(BT, C, HW)
    src = f32_in(R.to_channel_last(x), ld)
    n = BT * C * HW
    dst = f32_out(n)
    L.check(lb.ppms_nhwc_to_nchw(src.data_ptr(), ld, dst.data_ptr(), BT, C, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.Check(f"nhwc_to_nchw {case}").exact("dst", dst[:n].view(BT, C, HW), x))
    assert (dst[n:] == R.SENTINEL).all()
