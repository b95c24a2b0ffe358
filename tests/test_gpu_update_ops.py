"""GPU: the kernels that run inside every update iteration -- the correlation lookup (corr.hip), the correlation encoder's fused chains
and depthwise step (pwchain.hip, ppms_dwconv_gelu) and the block16 / SST attention helpers (attn16.hip: both the C = 384 / dh = 48 and the
C = 256 / dh = 32 instantiations) -- each called through the C ABI and compared with the plain float64 reference of tests/kernel_refs.py.

Tolerances as in test_gpu_encoder_ops.py (kernel_refs.py states the rule; none comes from the code under test); ppms_pwchain keeps the bounds
the suite already applies to it.  Inputs stored as split bf16 are rounded first, so that the reference sees what the kernel reads.  Every
output buffer holds a sentinel before the launch, padding channels of inputs hold junk, workspaces hold NaN."""
import ctypes as C

import pytest
import torch

import kernel_refs as R
from kernel_refs import f32_in, f32_out, planes_are, report, sp_in_junk, sp_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ correlation lookup
@pytest.mark.parametrize("case", list(R.LOOKUP_CASES))
def test_corr_lookup(lib, case):
    """ppms_corr_lookup on a pyramid uploaded as given (independent of ppms_corr_build), both kernels: the fp32 NCHW output with the flow in
    either layout; the SP output as the engine asks for it (flow_nhwc = 1) with out_ld 64 and 72, with and without the flow's SP copy at
    channels 254-255 of a 384-wide tensor.  Channels 36-63 zero, columns >= 64 untouched, the flow copy exactly sp_split(flow), its
    neighbours 253 and 256 untouched."""
    L, lb = lib, lib.load()
    B, H, W = R.LOOKUP_CASES[case]
    P = B * H * W
    levels, flow = R.lookup_inputs(case)
    lv = [t.to(DEV).contiguous() for t in levels]
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in lv])
    f_nhwc = flow.to(DEV).contiguous()
    f_nchw = flow.reshape(B, H, W, 2).permute(0, 3, 1, 2).contiguous().to(DEV)
    for nhwc, fd in ((0, f_nchw), (1, f_nhwc)):
        out = f32_out(P * 36)
        L.check(lb.ppms_corr_lookup(ptrs, fd.data_ptr(), nhwc, out.data_ptr(), None, None, 0, None, None, 0, B, H, W, L.stream_ptr()))
        torch.cuda.synchronize()
        got = out[:P * 36].view(B, 36, H, W).permute(0, 2, 3, 1).reshape(P, 36)
        report(R.lookup_check(case, got, False, f"corr_lookup {case} nchw flow_nhwc={nhwc}"))
        assert (out[P * 36:] == R.SENTINEL).all(), "written past (B, 36, H, W)"
    fhi, flo = R.sp_split(flow)
    for out_ld in (64, 72):
        for with_copy in (False, True):
            o, X = sp_out(L, P, out_ld), sp_out(L, P, 384)
            fl = X.view(254, 2)
            L.check(lb.ppms_corr_lookup(ptrs, f_nhwc.data_ptr(), 1, None, o.view().hi, o.view().lo, out_ld, fl.hi if with_copy else None,
                                        fl.lo if with_copy else None, 384, B, H, W, L.stream_ptr()))
            torch.cuda.synchronize()
            report(R.lookup_check(case, o.to_f32(0, 36), True, f"corr_lookup {case} sp ld={out_ld} copy={int(with_copy)}"))
            assert planes_are(o, 36, 64, 0.0), "channels 36-63 must be zero in both planes"
            assert planes_are(o, 64, out_ld, R.SENTINEL), "columns >= 64 must not be written"
            if with_copy:
                assert torch.equal(X.own()[0, :, 254:256].cpu(), fhi) and torch.equal(X.own()[1, :, 254:256].cpu(), flo), "flow copy != sp_split(flow)"
                assert planes_are(X, 0, 254, R.SENTINEL) and planes_are(X, 256, 384, R.SENTINEL), "written outside channels 254-255"
            else:
                assert planes_are(X, 0, 384, R.SENTINEL)


# ------------------------------------------------------------------------------------------------ depthwise k x k + residual GELU
@pytest.mark.parametrize("case", list(R.DWG_CASES))
def test_dwconv_gelu(lib, case):
    """ppms_dwconv_gelu: windows that cross the top and bottom of their frame and both row ends with BT > 1 and an odd W ("edges"); the
    engine's 40-channel view with junk in channels 40-63 of x; 64 channels with ld 72; k = 1.  Channels outside the view keep the sentinel."""
    L, lb = lib, lib.load()
    BT, H, W, c, ld, k = R.DWG_CASES[case]
    x, w, b = R.dwg_inputs(case)
    P = BT * H * W
    xs, ys = sp_in_junk(L, x.reshape(P, c), ld), sp_out(L, P, ld)
    wd, bd = w.to(DEV).contiguous(), b.to(DEV)
    L.check(lb.ppms_dwconv_gelu(xs.view(0, c), ys.view(0, c), wd.data_ptr(), bd.data_ptr(), k, BT, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.dwg_check(case, ys.to_f32(0, c).reshape(BT, H, W, c)))
    assert planes_are(ys, c, ld, R.SENTINEL), "channels outside the view must not be written"


def test_dwconv_gelu_refuses_misaligned_operands(lib):
    """16-byte loads of the bias and of the planes: a bias pointer one float in, and a view starting at channel 4, are refused before any
    launch; so are a null weight pointer and an empty map"""
    L, lb = lib, lib.load()
    BT, H, W, c, ld, k = R.DWG_CASES["edges"]
    x, w, b = R.dwg_inputs("edges")
    P = BT * H * W
    xs, ys = sp_in_junk(L, x.reshape(P, c), ld), sp_out(L, P, ld)
    wd, bd = w.to(DEV).contiguous(), b.to(DEV)
    bm = torch.zeros(c + 4, device=DEV)[1:c + 1]
    assert bm.data_ptr() % 16 == 4 and xs.view(4, 8).hi % 16 == 8
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(lb.ppms_dwconv_gelu(xs.view(0, c), ys.view(0, c), wd.data_ptr(), bm.data_ptr(), k, BT, H, W, L.stream_ptr()))
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(lb.ppms_dwconv_gelu(xs.view(4, 8), ys.view(0, c), wd.data_ptr(), bd.data_ptr(), k, BT, H, W, L.stream_ptr()))
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(lb.ppms_dwconv_gelu(xs.view(0, c), ys.view(4, 8), wd.data_ptr(), bd.data_ptr(), k, BT, H, W, L.stream_ptr()))
    with pytest.raises(RuntimeError, match="w and"):                          # no weights
        L.check(lb.ppms_dwconv_gelu(xs.view(0, c), ys.view(0, c), None, bd.data_ptr(), k, BT, H, W, L.stream_ptr()))
    with pytest.raises(RuntimeError, match="bad shape"):                      # an empty map
        L.check(lb.ppms_dwconv_gelu(xs.view(0, c), ys.view(0, c), wd.data_ptr(), bd.data_ptr(), k, BT, H, 0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert planes_are(ys, 0, ld, R.SENTINEL), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------ fused per-pixel chains
PW_ROWS = max(R.PW_PIXELS) + 3                                             # rows of every buffer: the rows beyond P must stay as they were


@pytest.fixture(scope="module")
def pw_packs(lib):
    """per chain: the packed layers as PwChain takes them (packed once, shared by the pixel counts)"""
    from ppmstereo_amd.packing import pack_conv2
    packs = {}
    for chain, (cin, spec, _) in R.PW_CHAINS.items():
        layers = []
        for (w, b, resid, post), (co, ci, _, _) in zip(R.pwchain_layers(chain), spec):
            pack = pack_conv2(w.reshape(co, ci, 1, 1).to(DEV), b.to(DEV), [ci], [64])
            M = pack[2]["M"]
            st = None
            if post is not None:
                st = (torch.zeros(M, device=DEV), torch.zeros(M, device=DEV))
                st[0][:co], st[1][:co] = post[0].to(DEV), post[1].to(DEV)
            layers.append((pack, co, resid, st))
        packs[chain] = layers
    return packs


@pytest.fixture(scope="module")
def pw_input(lib):
    """per input width: the SP input of all rows; channels >= cin hold junk (they meet zero weights)"""
    return {cin: sp_in_junk(lib, R.pwchain_input()[:, :cin].contiguous(), 64) for cin in (36, 64)}


def _pw_run(packs, xin, chain, P, out):
    from ppmstereo_amd.engine import PwChain
    PwChain(xin.view(0, 64), out.view(), packs[chain], P, [])()
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", R.PW_PIXELS)
@pytest.mark.parametrize("chain", list(R.PW_CHAINS))
def test_pwchain(lib, pw_packs, pw_input, chain, P):
    """ppms_pwchain: single layers (64 -> 64 with / without residual and post affine, 64 -> 256) at the project's conv bound, the engine's
    chains A and B at the bounds test_pwchain_vs_unfused_layers uses, against float64; 1, 318, 16384 (the last count of the 32-pixel-tile
    kernel) and 16385 pixels (the 128-pixel-tile kernel, one pixel in its last tile).  Rows >= P and channels >= n_valid of the output
    are not stored (include/ppms.h): they keep the sentinel."""
    L = lib
    cin, spec, _ = R.PW_CHAINS[chain]
    co, M = spec[-1][0], (spec[-1][0] + 63) // 64 * 64
    out = L.SPTensor(PW_ROWS, M + 8, DEV)
    out.data.fill_(R.SENTINEL)
    _pw_run(pw_packs, pw_input[cin], chain, P, out)
    report(R.pwchain_check(chain, P, out.to_f32(0, co)[:P]))
    d = out.own().float()
    assert (d[:, P:] == R.SENTINEL).all(), "rows beyond P must not be written"
    assert (d[:, :, co:] == R.SENTINEL).all(), "channels >= n_valid of the output are not stored"


def test_pwchain_two_kernels_same_bits(lib, pw_packs, pw_input):
    """pwchain.hip states that the 32-pixel-tile kernel gives the 128-pixel-tile kernel's results bit for bit: chain B on 16385 rows (the
    large kernel) and on the first 16384 rows of the same input (the small one) -- the operation is per pixel, so only the kernel differs"""
    L = lib
    big, small = sp_out(L, PW_ROWS, 256), sp_out(L, PW_ROWS, 256)
    _pw_run(pw_packs, pw_input[36], "B", 16385, big)
    _pw_run(pw_packs, pw_input[36], "B", 16384, small)
    assert torch.equal(big.own()[:, :16384], small.own()[:, :16384]), "the two pwchain kernels differ in some bit"
    assert (small.own()[:, 16384:].float() == R.SENTINEL).all() and (big.own()[:, 16385:].float() == R.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ time attention, LayerNorm (+ residual)
@pytest.mark.parametrize("data", R.A16_DATA)
@pytest.mark.parametrize("case", R.TA_CASES, ids=lambda c: f"T{c[0]}n{c[1]}")
@pytest.mark.parametrize("C", [256, 384])
def test_time_attn(lib, C, case, data):
    """ppms_time_attn, both instantiations, x and out views with ld = C + 8 (junk / sentinel in the padding), on unit data and on
    0.5 + 0.01 x, where the eps of the LayerNorm decides the result"""
    L, lb = lib, lib.load()
    T, n = case
    x, w, b = R.time_attn_inputs(C, case, data)
    xs, o = sp_in_junk(L, x.reshape(T * n, C), C + 8), sp_out(L, T * n, C + 8)
    wd, bd = w.to(DEV), b.to(DEV)
    L.check(lb.ppms_time_attn(xs.view(0, C), wd.data_ptr(), bd.data_ptr(), o.view(0, C), T, n, 8, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.time_attn_check(C, case, data, o.to_f32(0, C).reshape(T, n, C)))
    assert planes_are(o, C, C + 8, R.SENTINEL), "channels outside the view must not be written"


@pytest.mark.parametrize("C,T,message", [(384, R.TA_MAX_T[384] + 1, "more than 64 KiB"), (384, 64, "more than 64 KiB"),
                                         (256, R.TA_MAX_T[256] + 1, "bad T")])           # (256, 65): the limit T <= 64 the entry point always had
def test_time_attn_refuses_more_frames_than_its_lds_holds(lib, C, T, message):
    """T * C * 4 bytes of LDS above 64 KiB (T > 42 at C = 384; T > 64 at C = 256): refused with PPMS_EINVAL and the refusal's own
    message -- a failed launch would raise too, with another text --, never launched"""
    L, lb = lib, lib.load()
    xs, o = sp_out(L, T, C), sp_out(L, T, C)
    wd = torch.ones(C, device=DEV)
    rc = lb.ppms_time_attn(xs.view(), wd.data_ptr(), wd.data_ptr(), o.view(), T, 1, 8, L.stream_ptr())
    assert rc == -1, f"PPMS_EINVAL expected, got {rc}"
    with pytest.raises(RuntimeError, match=message):
        L.check(rc)
    torch.cuda.synchronize()
    assert planes_are(o, 0, C, R.SENTINEL), "a refused call must not launch"


@pytest.mark.parametrize("C", [256, 384])
def test_time_attn_at_the_largest_accepted_T(lib, C):
    """the boundary from the other side: T = 42 at C = 384 (64 512 bytes of LDS) and T = 64 at C = 256 (exactly 64 KiB) are served, one
    pixel, against the float64 reference"""
    L, lb = lib, lib.load()
    case = (R.TA_MAX_T[C], 1)
    T, n = case
    assert T * C * 4 <= 65536 < (T + 1) * C * 4
    x, w, b = R.time_attn_inputs(C, case, "unit")
    xs, o = sp_in_junk(L, x.reshape(T * n, C), C + 8), sp_out(L, T * n, C + 8)
    wd, bd = w.to(DEV), b.to(DEV)
    L.check(lb.ppms_time_attn(xs.view(0, C), wd.data_ptr(), bd.data_ptr(), o.view(0, C), T, n, 8, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.time_attn_check(C, case, "unit", o.to_f32(0, C).reshape(T, n, C)))
    assert planes_are(o, C, C + 8, R.SENTINEL), "channels outside the view must not be written"


@pytest.mark.parametrize("data", R.A16_DATA)
@pytest.mark.parametrize("C", [256, 384])
def test_layernorm(lib, C, data):
    """ppms_layernorm, both instantiations: 231 pixels (a 4-pixel-block tail of 3), x with ld = C + 4, without a residual and with a
    residual view whose ld (C + 16) differs from the output's (C + 8)"""
    L, lb = lib, lib.load()
    P = R.LN16_PIXELS
    x, w, b, res = R.layernorm16_inputs(C, data)
    xd, wd, bd = f32_in(x, C + 4), w.to(DEV), b.to(DEV)
    rs = sp_in_junk(L, res, C + 16)
    for with_res in (False, True):
        o = sp_out(L, P, C + 8)
        rv = rs.view(0, C) if with_res else L.SP(None, None, 0, 0)
        L.check(lb.ppms_layernorm(xd.data_ptr(), C + 4, wd.data_ptr(), bd.data_ptr(), rv, o.view(0, C), P, C, L.stream_ptr()))
        torch.cuda.synchronize()
        report(R.layernorm16_check(C, data, with_res, o.to_f32(0, C)))
        assert planes_are(o, C, C + 8, R.SENTINEL), "channels outside the view must not be written"


# ------------------------------------------------------------------------------------------------ linear attention
@pytest.mark.parametrize("data", R.LA_DATA)
@pytest.mark.parametrize("case", R.LA_CASES, ids=lambda c: f"T{c[0]}n{c[1]}")
@pytest.mark.parametrize("dh", [32, 48])
def test_linear_attention(lib, dh, case, data):
    """ppms_linear_attention, both instantiations: an empty pixel split (n = 3), a 32-pixel apply tail of 13, a share of 161 = one 160-pixel
    pass plus one pixel; three contiguous buffers, the engine's layout (Q | K in one buffer of ld 2 C) and the SST's (K | V in one buffer);
    the workspace holds NaN before the launch; unit-scale K, and K x 1e-6, where the 1e-6 of the divisor shows"""
    L, lb = lib, lib.load()
    T, n = case
    Cc, P = 8 * dh, T * n
    Q, K, V = (t.reshape(P, Cc).to(DEV) for t in R.linattn_inputs(dh, case, data))
    nws = int(lb.ppms_linear_attention_workspace_floats(T, n, 8, dh))
    for layout in ("contiguous", "qk", "kv"):
        if layout == "qk":
            pair = torch.cat([Q, K], 1)
            ops = (pair, 2 * Cc, pair[:, Cc:], 2 * Cc, V.contiguous(), Cc)
        elif layout == "kv":
            pair = torch.cat([K, V], 1)
            ops = (Q.contiguous(), Cc, pair, 2 * Cc, pair[:, Cc:], 2 * Cc)
        else:
            ops = (Q.contiguous(), Cc, K.contiguous(), Cc, V.contiguous(), Cc)
        ws = torch.full((nws + 4,), NAN, device=DEV)
        o = sp_out(L, P, Cc + 8)
        L.check(lb.ppms_linear_attention(ops[0].data_ptr(), ops[1], ops[2].data_ptr(), ops[3], ops[4].data_ptr(), ops[5], ws.data_ptr(), o.view(0, Cc),
                                         T, n, 8, dh, L.stream_ptr()))
        torch.cuda.synchronize()
        report(R.linattn_check(dh, case, data, o.to_f32(0, Cc).reshape(T, n, 8, dh), f"linear_attention dh={dh} T,n={case} {data} {layout}"))
        assert planes_are(o, Cc, Cc + 8, R.SENTINEL), "channels outside the view must not be written"
        assert torch.isfinite(ws[:nws]).all() and torch.isnan(ws[nws:]).all(), "every partial of the workspace is written, nothing behind it"
