"""GPU: the non-convolution kernels of the two encoders (encoder_ops.hip), each called through the C ABI and compared with the plain
float64 reference of tests/kernel_refs.py at the smallest shapes that reach each of its branches.

Tolerances (kernel_refs.py states the rule; none comes from the code under test): (a) exact -- torch.equal on the planes -- for copies and
permutations and for the hi plane of a split; (b) 2e-5 * max(1, max|ref|) for split-bf16 outputs of elementwise math; (c) for reductions
and transcendentals 8 x the max error of the same operation in plain fp32 torch on the CPU on the same input, or (b) where the output
is split bf16, whichever is larger.  Inputs stored as split bf16 are read back with to_f32() so that the reference sees exactly what the
kernel sees.  Every output buffer is pre-filled with a sentinel (1.0 in both planes / in the fp32 buffer): after the launch the padding
channels of the view are zero where the kernel promises zero fill, and everything outside the view still holds the sentinel."""
import pytest
import torch

import kernel_refs as R
from kernel_refs import f32_in, f32_out, planes_are, report, sp_in, sp_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ InstanceNorm
@pytest.mark.parametrize("data", ["unit", "offset"])
@pytest.mark.parametrize("case", list(R.INSTNORM_CASES))
def test_instnorm(lib, case, data):
    """ppms_instnorm_stats + ppms_instnorm_apply: the stats array and the applied result, with relu 0 / 1, with and without a residual, on
    unit data (catches an unbiased variance) and on 50 + 0.05 x (catches eps 1e-6 and a one-pass variance).  A: S = 66 slices, one empty,
    merge groups ending in a tail of 2; B: S = 1 with a ragged tail; C: last channel block 8 wide, ld != C, S = 10; D: the scalar paths of
    part and apply (ld = 31, C = 30, x not 16-B aligned), out channels 30 and 31 zero."""
    L, lb = lib, lib.load()
    N, C, HW, ld, outc, misaligned = R.INSTNORM_CASES[case]
    x, res = R.instnorm_inputs(case, data)
    P, C8 = N * HW, (C + 7) // 8 * 8
    xd = f32_in(x.reshape(P, C), ld, misaligned)
    rs = sp_in(L, res.reshape(P, C8))
    stats = f32_out(N * C * 2)
    ws = torch.full((max(int(lb.ppms_instnorm_workspace_bytes(N, HW, C)) // 4, 4),), float("nan"), device=DEV)
    L.check(lb.ppms_instnorm_stats(xd.data_ptr(), ld, N, HW, C, R.IN_EPS, stats.data_ptr(), ws.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    st = stats[:N * C * 2].view(N, C, 2).cpu()
    assert (stats[N * C * 2:] == R.SENTINEL).all(), "stats written past N * C pairs"
    for with_res in (False, True):
        for relu in (0, 1):
            out = sp_out(L, P, outc + 8)
            rv = rs.view(0, C8) if with_res else L.SP(None, None, 0, 0)
            L.check(lb.ppms_instnorm_apply(xd.data_ptr(), ld, stats.data_ptr(), rv, relu, out.view(0, outc), N, HW, C, L.stream_ptr()))
            torch.cuda.synchronize()
            y = out.to_f32(0, C).reshape(N, HW, C)
            report(R.instnorm_check(case, data, with_res, bool(relu), st[..., 0], st[..., 1], y))
            assert planes_are(out, C, outc, 0.0), "padding channels of the view must be zero"
            assert planes_are(out, outc, outc + 8, R.SENTINEL), "channels outside the view must not be written"


def test_instnorm_stats_refuses_a_misaligned_workspace(lib):
    """the per-slice records are 16 bytes, stored and loaded whole: a workspace that is not 16-B aligned is refused before any launch"""
    L, lb = lib, lib.load()
    N, C, HW, ld, _, _ = R.INSTNORM_CASES["B"]
    xd = f32_in(R.instnorm_inputs("B", "unit")[0].reshape(N * HW, C), ld)
    stats = f32_out(N * C * 2)
    ws = torch.zeros(int(lb.ppms_instnorm_workspace_bytes(N, HW, C)) // 4 + 4, device=DEV)[1:]
    assert ws.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(lb.ppms_instnorm_stats(xd.data_ptr(), ld, N, HW, C, R.IN_EPS, stats.data_ptr(), ws.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert (stats == R.SENTINEL).all() and (ws == 0).all(), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------ GRN
@pytest.mark.parametrize("case", list(R.GRN_CASES))
def test_grn(lib, case):
    """ppms_grn: small; a 66-slice map with an empty slice; C = 3072 (the merge's loop over C > 256, S = 2); inputs of magnitude 2e-6 with
    gamma scaled by 1 / max|x| (the only case where the 1e-6 of the divisor shows); ld % 4 != 0 (scalar paths of part and apply).  The out
    view is 8 channels wider than C: GRN writes C channels only, the rest keep the sentinel."""
    L, lb = lib, lib.load()
    N, HW, C, ld, _ = R.GRN_CASES[case]
    h, gamma, beta = R.grn_inputs(case)
    P = N * HW
    xd = f32_in(h.reshape(P, C), ld)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    out = sp_out(L, P, C + 16)
    ws = torch.full((int(lb.ppms_grn_workspace_bytes(N, HW, C)) // 4,), float("nan"), device=DEV)
    L.check(lb.ppms_grn(xd.data_ptr(), ld, gd.data_ptr(), bd.data_ptr(), out.view(0, C + 8), N, HW, C, ws.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.grn_check(case, out.to_f32(0, C).reshape(N, HW, C)))
    assert planes_are(out, C, C + 16, R.SENTINEL), "GRN writes C channels only"


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("C", list(R.LN_CASES))
def test_layernorm_any(lib, C, pad):
    """ppms_layernorm_any on 37 pixels (not a multiple of the 4 of a workgroup), eps 1e-6, ld = C and C + 4: every third row scaled by
    1e-2, every third row plus one is 20 + 0.3 x.  C = 520: second round with one active lane; 1024: the limit; 36 into a 40-channel view:
    the scalar path, channels 36-39 zero."""
    L, lb = lib, lib.load()
    x, w, b = R.layernorm_inputs(C)
    outc, P = R.LN_CASES[C], R.LN_PIXELS
    xd = f32_in(x, C + pad)
    wd, bd = w.to(DEV), b.to(DEV)
    out = sp_out(L, P, outc + 8)
    L.check(lb.ppms_layernorm_any(xd.data_ptr(), C + pad, wd.data_ptr(), bd.data_ptr(), R.LN_EPS, out.view(0, outc), P, C, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.layernorm_check(C, out.to_f32(0, C)))
    assert planes_are(out, C, outc, 0.0), "padding channels of the view must be zero"
    assert planes_are(out, outc, outc + 8, R.SENTINEL), "channels outside the view must not be written"


def test_layernorm_any_refuses_more_than_1024_channels(lib):
    L, lb = lib, lib.load()
    x, w, b = R.layernorm_inputs(1024)
    xd, wd, bd = f32_in(x, 1024), w.to(DEV), b.to(DEV)
    out = sp_out(L, R.LN_PIXELS, 1040)
    with pytest.raises(RuntimeError):
        L.check(lb.ppms_layernorm_any(xd.data_ptr(), 1024, wd.data_ptr(), bd.data_ptr(), R.LN_EPS, out.view(0, 1032), R.LN_PIXELS, 1024, L.stream_ptr()))
    torch.cuda.synchronize()
    assert planes_are(out, 0, 1040, R.SENTINEL)


# ------------------------------------------------------------------------------------------------ depthwise 7 x 7
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv(lib, case, pad):
    """ppms_dwconv, ldy = C and C + 4: a last channel block of 32 channels with W < 4 (2, 1, 2, 96); W % 4 != 0 with whole blocks; 12
    blocks; whole runs.  The fp32 output: tolerance kind (c)."""
    L, lb = lib, lib.load()
    N, H, W, C = case
    x, w, b = R.dwconv_inputs(case)
    P, ldy = N * H * W, C + pad
    xs = sp_in(L, x.reshape(P, C))
    wd, bd = w.to(DEV), b.to(DEV)
    y = f32_out(P * ldy)
    L.check(lb.ppms_dwconv(xs.view(0, C), y.data_ptr(), ldy, wd.data_ptr(), bd.data_ptr(), 7, N, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    got = y[:P * ldy].view(P, ldy).cpu()
    report(R.dwconv_check(case, got[:, :C].reshape(N, H, W, C)))
    assert (got[:, C:] == R.SENTINEL).all() and (y[P * ldy:] == R.SENTINEL).all(), "columns outside the C channels must not be written"


def test_dwconv_refusals(lib):
    """k = 3, and a bias that is not 16-B aligned (the kernel loads it 16 bytes at a time): refused before any launch"""
    L, lb = lib, lib.load()
    N, H, W, C = R.DW_CASES[0]
    x, w, b = R.dwconv_inputs(R.DW_CASES[0])
    P = N * H * W
    xs = sp_in(L, x.reshape(P, C))
    wd, bd = w.to(DEV), b.to(DEV)
    y = f32_out(P * C)
    with pytest.raises(RuntimeError):
        L.check(lb.ppms_dwconv(xs.view(0, C), y.data_ptr(), C, wd.data_ptr(), bd.data_ptr(), 3, N, H, W, L.stream_ptr()))
    bm = torch.zeros(C + 4, device=DEV)[1:C + 1]
    assert bm.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(lb.ppms_dwconv(xs.view(0, C), y.data_ptr(), C, wd.data_ptr(), bm.data_ptr(), 7, N, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (y == R.SENTINEL).all(), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------ layout kernels: exact
def test_sp_upsample2(lib):
    """nearest x2 of a 16-channel view at channel 8 of a 32-channel tensor: both planes bitwise"""
    L, lb = lib, lib.load()
    N, H, W = R.UP_CASE
    src = sp_in(L, R.upsample_input(), extra=0)
    dst = sp_out(L, N * 4 * H * W, 32)
    L.check(lb.ppms_sp_upsample2(src.view(8, 16), dst.view(8, 16), N, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    for pl in range(2):
        want = R.upsample2(src.own()[pl].cpu().reshape(N, H, W, 32)[..., 8:24]).reshape(-1, 16)
        assert torch.equal(dst.own()[pl, :, 8:24].cpu(), want)
    assert planes_are(dst, 0, 8, R.SENTINEL) and planes_are(dst, 24, 32, R.SENTINEL)


@pytest.mark.parametrize("case", R.S2D_CASES, ids=lambda c: f"C{c[3]}")
def test_sp_s2d(lib, case):
    L, lb = lib, lib.load()
    N, H, W, C = case
    src = sp_in(L, R.s2d_input(case))
    dst = sp_out(L, N * H * W // 4, 4 * C + 8)
    L.check(lb.ppms_sp_s2d(src.view(0, C), dst.view(0, 4 * C), N, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    for pl in range(2):
        want = R.s2d(src.own()[pl, :, :C].cpu().reshape(N, H, W, C), 2).reshape(-1, 4 * C)
        assert torch.equal(dst.own()[pl, :, :4 * C].cpu(), want)
    assert planes_are(dst, 4 * C, 4 * C + 8, R.SENTINEL)
    with pytest.raises(RuntimeError):                                          # odd H
        L.check(lb.ppms_sp_s2d(src.view(0, C), dst.view(0, 4 * C), N, H - 1, W, L.stream_ptr()))


@pytest.mark.parametrize("case", R.IMG_S2D_CASES, ids=[f"k{c[0]}_c{c[2]}" for c in R.IMG_S2D_CASES])
def test_img_s2d(lib, case):
    """the fp32 NCHW image to the split planes of its space-to-depth copy: hi = bf16(x) exactly, |hi + lo - x| <= 2^-16 |x| (each of the two
    roundings to 8 significant bits costs at most 2^-8 relative), channels >= k k C of the view zero"""
    L, lb = lib, lib.load()
    k, shape, dc = case
    N, C, H, W = shape
    img = R.img_input(shape)
    imd = img.to(DEV)
    P = N * (H // k) * (W // k)
    dst = sp_out(L, P, dc + 8)
    L.check(lb.ppms_img_s2d(imd.data_ptr(), dst.view(0, dc), N, C, H, W, k, L.stream_ptr()))
    torch.cuda.synchronize()
    want = R.s2d(img.permute(0, 2, 3, 1), k).reshape(P, k * k * C)
    d = dst.own().cpu()
    report(R.split_check(R.Check(f"img_s2d k={k} dst.c={dc}"), "planes", d[0, :, :k * k * C], d[1, :, :k * k * C], want))
    assert planes_are(dst, k * k * C, dc, 0.0), "padding channels of the view must be zero"
    assert planes_are(dst, dc, dc + 8, R.SENTINEL)
    with pytest.raises(RuntimeError):                                          # H not a multiple of k
        L.check(lb.ppms_img_s2d(imd.data_ptr(), dst.view(0, dc), N, C, H - 1, W, k, L.stream_ptr()))
