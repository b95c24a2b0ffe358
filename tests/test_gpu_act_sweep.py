"""GPU: the fused activations and epilogue kinds of every conv kernel, isolated from the GEMM and swept over their whole input range
against float64 (tests/act_sweep.py has the construction, the grid, the references and the bound 2^-20 max(1, |pre|, |aux|, |ref|)).

Per (kernel, shape): ACT_NONE first -- out_f32 must be the injected values bit for bit, which proves the construction on that kernel --,
then every epilogue class the kernel instantiates: PLAIN with the six activations and scale = 0.25, PRE, AUX, AUXPRE, GRU with and without the
hoisted share, and ANY with out_vt where the kernel serves it.  NaN goes through every launch in one cout (the last valid one: inside the
ragged 4-wide tail where there is one), +-inf through the STORE launches of NONE / RELU / SIGMOID / TANH; both must come out exactly.
Not swept: gelu(-inf) (-inf * 0) and +-inf through SP outputs (split_bf16(inf) has lo = NaN by construction).

Every launch also shows: nothing written outside the valid couts and the output rows (sentinels around and inside the buffers), every
expected element written (no sentinel left), the same bits from a second launch, the SP planes consistent with out_f32 of the same launch
(hi == bf16(out_f32), |hi + lo - out_f32| <= 2^-16 |out_f32| + 2^-133), and V^T equal to vt_enc(out_f32) in both formats.
The 2^-133 is bf16's smallest step: sigmoid and elu + 1 reach down to 1e-38 and below, where lo = bf16(out - hi) is a denormal and each of the
two roundings costs up to half of that step instead of 2^-8 relative (plain IEEE arithmetic on the CPU shows the same 4.5e-41)."""
import pytest
import torch

import act_sweep as S
from act_sweep import Half, Kernel, Site
from ppmstereo_amd import _lib as L
from ppmstereo_amd.packing import CONV2, CONV5, CONV6, GEMM1

pytestmark = pytest.mark.gpu
SENT_BF16 = torch.tensor([S.SENT]).to(torch.bfloat16).float().item()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    return L


def _check(label, o):
    """one epilogue half of one launch against the reference, and its outputs against each other"""
    hf, got, n = o["half"], o["f32"], o["half"].n_valid
    assert o["intact"], f"{label}: written outside the valid couts / rows of an output"
    assert o["same"], f"{label}: a second launch gave other bits"
    assert not (got == S.SENT).any(), f"{label}: out_f32 elements not written"
    out = S.compare(label, hf.kind, hf.act, hf.scale, got, o["v"], o.get("aux"), o.get("z"))
    print("SWEEP", out)
    tail = n // 8 * 8
    if tail < n:                                                            # the ragged couts run the 4-wide predicated form: its own figure
        cut = lambda t: None if t is None else t[:, tail:]
        print("SWEEP", S.compare(label + " [4-wide tail]", hf.kind, hf.act, hf.scale, got[:, tail:], o["v"][:, tail:], cut(o.get("aux")), cut(o.get("z"))))
    assert out.ok, str(out)
    nan_c = S.special_couts(n)["nan"]
    assert torch.isnan(got[:, nan_c]).all() and not torch.isnan(got[:, :nan_c]).any(), f"{label}: NaN in, NaN out, in that cout alone"
    if "hi" in o:
        hi, lo = o["hi"], o["lo"]
        assert not (hi.float() == SENT_BF16).any(), f"{label}: out_sp elements not written"
        keep = ~torch.isinf(got)                                            # (inf: lo = inf - inf)
        assert S.same_bits(hi.float(), got.to(torch.bfloat16).float())[keep].all(), f"{label}: hi plane != bf16(out_f32)"
        fin = torch.isfinite(got)
        over = ((hi.double() + lo.double() - got.double()).abs() - (got.double().abs() * 2.0 ** -16 + 2.0 ** -133))[fin]
        i = int(over.argmax())
        assert over[i] <= 0, f"{label}: |hi + lo - out_f32| > 2^-16 |out_f32| + 2^-133 at out_f32 = {got[fin][i].item()!r}: hi {hi[fin][i].item()!r} lo {lo[fin][i].item()!r}"
    if "vt" in o:
        T = o["vt"].shape[0]
        want = S.vt_bits(got.reshape(T, -1, n).permute(0, 2, 1).contiguous(), hf.vt)
        dec = lambda b: L.vt_values(b.view(torch.bfloat16), hf.vt)
        assert S.same_bits(dec(o["vt"].view(torch.int16)), dec(want)).all(), f"{label}: V^T != vt_enc(out_f32), vt_f16 = {hf.vt}"
    return out


def _classes(n):
    """(class, Half) of the full sweep of one kernel at n couts; ACT_NONE first"""
    G, SG, TH = L.ACT_GELU, L.ACT_SIGMOID, L.ACT_TANH
    yield from ((f"PLAIN {S.ACT_NAMES[a]}", Half(n, act=a)) for a in S.ACTS)
    yield "PLAIN scale=0.25", Half(n, scale=0.25)
    yield "PRE none", Half(n, pre=True)
    yield "PRE gelu", Half(n, act=G, pre=True)
    yield "PRE sigmoid", Half(n, act=SG, pre=True)
    yield "AUX resid+gelu", Half(n, L.EPI_RESID, G)
    yield "AUX resid+relu", Half(n, L.EPI_RESID, L.ACT_RELU)
    yield "AUX rh", Half(n, L.EPI_RH)
    yield "AUXPRE rh", Half(n, L.EPI_RH, pre=True)
    yield "GRU", Half(n, L.EPI_GRU)
    yield "GRU pre", Half(n, L.EPI_GRU, pre=True)


def _sweep(sid):
    st = S.site(sid)
    assert st.grid_fits()
    n = st.couts[0]
    for cls, hf in _classes(n):
        label = f"{sid} | {st.kernel} | {cls}"
        if hf.pre and n % 4:                                                # the one refusal of the sweep: the share is read four couts at a time
            why = S.refusal(lambda: st.run([hf]))
            assert "must be a multiple of 4 with pre_f32" in why, f"{label}: {why!r}"
            continue
        out = _check(label, st.run([hf])[0])
        if hf.act == L.ACT_NONE and hf.kind == L.EPI_STORE and hf.scale == 1.0:
            assert out.ok and out.err == 0.0, f"{label}: the injection is not exact on this kernel"


def _sites_of(prefix):
    return [s for s in S.SITES if s.startswith(prefix)]


@pytest.mark.parametrize("sid", _sites_of("conv_gemm2"))
def test_conv_gemm2(lib, sid):
    """both wave layouts at 64 and ragged 54 couts (row8_finish and the 4-wide epilogue_group), the y-swept form, and a K-sliced launch
    whose epilogue runs in the slice-reduce kernel (epilogue_row8) at ragged 190 couts"""
    _sweep(sid)


@pytest.mark.parametrize("sid", _sites_of("conv_stream"))
def test_conv_stream(lib, sid):
    _sweep(sid)


@pytest.mark.parametrize("sid", _sites_of("conv_gemm5"))
def test_conv_gemm5(lib, sid):
    """7 and 8 pixel blocks per tile; 128 couts (both K-groups run the epilogue on swapped halves), 256, ragged 190"""
    _sweep(sid)


@pytest.mark.parametrize("sid", _sites_of("conv_gemm6"))
def test_conv_gemm6(lib, sid):
    _sweep(sid)


@pytest.mark.parametrize("sid", _sites_of("gemm1"))
def test_gemm1(lib, sid):
    _sweep(sid)


@pytest.mark.parametrize("M,n0,n1", [(256, 128, 128), (192, 126, 64)])
def test_conv_gemm6_two_halves(lib, M, n0, n1):
    """different epilogues in epi[0] and epi[1] of one launch (m_split = 128; with M = 192 wave 2's couts straddle the split)"""
    st = Site(Kernel("conv_gemm6", CONV6, m_pad=M), 2, 20, 30, 64, [n0, n1], (1, 3, 3), m_split=128, cout_map=list(range(n0)) + list(range(128, 128 + n1)))
    for a, b in ((Half(n0), Half(n1)), (Half(n0, act=L.ACT_GELU), Half(n1, act=L.ACT_TANH)), (Half(n0, act=L.ACT_SIGMOID), Half(n1, act=L.ACT_ELU1)),
                 (Half(n0, L.EPI_GRU), Half(n1, L.EPI_RH)), (Half(n0, act=L.ACT_RELU, f32=True, sp=True), Half(n1, L.EPI_RESID, L.ACT_GELU))):
        outs = st.run([a, b])
        for h, o in enumerate(outs):
            hf = o["half"]
            _check(f"conv_gemm6 two halves M={M} | epi[{h}] {S.KIND_NAMES[hf.kind]} {S.ACT_NAMES[hf.act]}", o)


def test_gemm1_elu1_at_768_couts(lib):
    """the linear attention's q | k projection: elu + 1 over 768 couts into fp32, the v half scaled, in one launch"""
    st = Site(Kernel("gemm1", GEMM1), 2, 8, 32, 384, [768, 384], (1, 1, 1), m_split=768)
    outs = st.run([Half(768, sp=False), Half(384, sp=False)])
    for h, o in enumerate(outs):
        assert _check(f"gemm1 768|384 | epi[{h}] none", o).err == 0.0
    outs = st.run([Half(768, act=L.ACT_ELU1, sp=False), Half(384, scale=0.5, sp=False)])
    _check("gemm1 768|384 | epi[0] PLAIN elu1", outs[0])
    _check("gemm1 768|384 | epi[1] PLAIN scale=0.5", outs[1])


VT_SITES = {  # kernel, T, H, W, cin, cout: each kernel that writes V^T, on a map with W % 8 == 0 and on one without
    "conv_gemm2-w10-54": (Kernel("conv_gemm2 V^T from the accumulators", CONV2), 2, 6, 10, 64, 54),
    "conv_gemm2-w32-64": (Kernel("conv_gemm2 V^T from the staged patch", CONV2), 2, 8, 32, 64, 64),
    "conv_gemm5-w64-128": (Kernel("conv_gemm5 V^T", CONV5), 2, 12, 64, 64, 128),
    "conv_gemm5-w60-128": (Kernel("conv_gemm5 V^T", CONV5), 2, 12, 60, 64, 128),
    "gemm1-w32-128": (Kernel("gemm1 V^T", GEMM1), 2, 8, 32, 128, 128),
    "gemm1-w7-128": (Kernel("gemm1 V^T", GEMM1), 1, 5, 7, 128, 128),
    "gemm1-w40-54": (Kernel("gemm1 V^T", GEMM1), 3, 5, 40, 256, 54),
}


@pytest.mark.parametrize("vid", list(VT_SITES))
def test_out_vt(lib, vid):
    """EPI_CLS_ANY with out_vt: the stored 16 bits are vt_enc of that launch's out_f32 -- bf16(y), or its fp16 image saturated at +-65504 --
    for both vt_f16 values; ACT_NONE on inputs with +-65504, +-65520, +-1e5 and NaN, then GELU and TANH on the grid (each V^T form applies the
    activation itself)."""
    k, T, H, W, cin, n = VT_SITES[vid]
    st = Site(k, T, H, W, cin, [n], (1, 1, 1) if k.version == GEMM1 else (1, 3, 3), extra=S.VT_VALUES)
    for fmt in (L.ATTN_P_BF16, L.ATTN_P_FP16):
        for act in (L.ACT_NONE, L.ACT_GELU, L.ACT_TANH):
            o = st.run([Half(n, act=act, vt=fmt)])[0]
            out = _check(f"{vid} | {k} | ANY+out_vt {S.ACT_NAMES[act]} vt_f16={fmt}", o)
            if act == L.ACT_NONE:
                assert out.err == 0.0
                held = set(o["f32"][1].tolist())
                assert all(v in held for v in S.VT_VALUES), "the saturation inputs must reach the encoder"


def test_out_vt_is_refused_where_no_kernel_writes_it(lib):
    """conv_stream and conv_gemm6 do not serve out_vt (conv_check.h), nor does a K-sliced conv_gemm2 launch: each says so"""
    from ppmstereo_amd.packing import STREAM
    for k, T, H, W, cin, n, msg in ((Kernel("conv_stream", STREAM), 2, 6, 10, 64, 64, "out_vt is not served"),
                                    (Kernel("conv_gemm6", CONV6, m_pad=128), 2, 12, 64, 64, 128, "out_vt is not served"),
                                    (Kernel("conv_gemm2 sliced", CONV2, nslice=3), 2, 6, 10, 64, 64, "cannot write out_vt")):
        st = Site(k, T, H, W, cin, [n], (1, 3, 3))
        why = S.refusal(lambda: st.run([Half(n, vt=L.ATTN_P_FP16)]))
        assert msg in why, (str(k), why)


# ------------------------------------------------------------------------------------------------ the same functions outside the convs
@pytest.mark.parametrize("k", list(S.DWG_SWEEP))
def test_dwconv_gelu_sweep(lib, k):
    """ppms_dwconv_gelu with zero depthwise weights and bias is gelu(x): the 16-bit grid through gelu_erf at this call site; the output is
    split bf16, so the bound is the storage's 2^-16 |ref| on top of the activation's: 2^-16 |ref| + 2^-20 max(1, |x|) per element"""
    import kernel_refs as R
    BT, H, W, c, ld = S.DWG_SWEEP[k]
    P = BT * H * W
    x = S.dwg_sweep_input(k)
    xs, ys = R.sp_in_junk(L, x.reshape(P, c), ld), R.sp_out(L, P, ld)
    wd, bd = torch.zeros(c, k * k, device=S.GPU), torch.zeros(c, device=S.GPU)
    L.check(L.load().ppms_dwconv_gelu(xs.view(0, c), ys.view(0, c), wd.data_ptr(), bd.data_ptr(), k, BT, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    got = ys.to_f32(0, c).cpu().double().reshape(BT, H, W, c)
    ref = R.dwconv_gelu(x, wd.cpu(), bd.cpu(), k)
    err, tol = (got - ref).abs(), S.storage_bound(ref, x)
    i = int((err / tol).argmax())
    print(f"SWEEP dwconv_gelu k={k}: max err/bound {(err / tol).flatten()[i].item():.3f}, err {err.flatten()[i].item():.3e} at x = {x.flatten()[i].item()!r}")
    assert torch.isfinite(got).all() and (err <= tol).all(), f"x = {x.flatten()[i].item()!r}: {got.flatten()[i].item()!r} vs {ref.flatten()[i].item()!r}"
    assert R.planes_are(ys, c, ld, R.SENTINEL), "channels outside the view must not be written"


@pytest.mark.parametrize("P", [5 * 7 * 9 + 3, 16384 + 128 + 5])
def test_pwchain_gelu_sweep(lib, P):
    """ppms_pwchain, both kernels (318 rows: 32-pixel tiles; 16517: 128-pixel tiles, the counts of test_pwchain_vs_unfused_layers), on a
    one-layer 64 -> 64 chain with IDENTITY weights and zero bias: the layer's sum is exactly x, so the output is gelu(x) of the 16-bit grid
    and the bound is the activation's plus the storage's, 2^-16 |ref| + 2^-20 max(1, |x|) per element, against kernel_refs.pwchain.
    (With dense weights the layer's own bf16x3 error, ~2^-18 sum |w x|, is tens of times this bound wherever the sum cancels: such a chain
    says nothing about the activation, and tests/test_gpu_update_ops.py already checks those at the conv bound.)"""
    import kernel_refs as R
    from ppmstereo_amd.engine import PwChain
    from ppmstereo_amd.packing import pack_conv2
    x = S.layout(S.GRID16, P, 64)
    w, b = torch.eye(64), torch.zeros(64)
    xs, out = R.sp_in(L, x, extra=0), R.sp_out(L, P + 3, 72)
    PwChain(xs.view(0, 64), out.view(0, 64), [(pack_conv2(w.reshape(64, 64, 1, 1).to(S.GPU), b.to(S.GPU), [64], [64]), 64, False, None)], P, [])()
    torch.cuda.synchronize()
    got = out.to_f32(0, 64)[:P].cpu().double()
    ref = R.pwchain(x, [(w, b, False, None)])
    err, tol = (got - ref).abs(), S.storage_bound(ref, x)
    i = int((err / tol).argmax())
    print(f"SWEEP pwchain P={P}: max err/bound {(err / tol).flatten()[i].item():.3f}, err {err.flatten()[i].item():.3e} at x = {x.flatten()[i].item()!r}")
    assert torch.isfinite(got).all() and (err <= tol).all(), f"x = {x.flatten()[i].item()!r}: {got.flatten()[i].item()!r} vs {ref.flatten()[i].item()!r}"
    d = out.own().float()
    assert (d[:, P:] == R.SENTINEL).all() and (d[:, :, 64:] == R.SENTINEL).all(), "rows beyond P and channels beyond the view must not be written"


def _convex(case, T, H, W, taps, t_halo, seed):
    import kernel_refs as R
    from ppmstereo_amd.weights import hash_normal
    P, HW, ld = T * H * W, H * W, taps * 16 + 8
    fl = hash_normal((T + 2 * t_halo, H, W, 2), seed)
    m = S.convex_logits(case, P, taps, seed + 1)
    fd = torch.full(((T + 2 * t_halo) * HW * 2 + 16,), R.JUNK, device=S.GPU)
    fd[8:8 + fl.numel()] = fl.reshape(-1).to(S.GPU)
    own = fd[8 + t_halo * HW * 2:]
    md = R.f32_in(m, ld)                                                    # JUNK in the padding columns
    out = R.f32_out(T * 2 * 16 * HW)
    lb = L.load()
    if taps == 9:
        L.check(lb.ppms_convex_upsample(own.data_ptr(), md.data_ptr(), ld, out.data_ptr(), T, H, W, L.stream_ptr()))
    else:
        L.check(lb.ppms_convex_upsample_3d(own.data_ptr(), md.data_ptr(), ld, out.data_ptr(), T, H, W, t_halo, L.stream_ptr()))
    torch.cuda.synchronize()
    m4 = m.reshape(T, H, W, taps * 16)
    ref, f32 = S.convex_upsample(fl, m4, t_halo), S.convex_upsample(fl, m4, t_halo, torch.float32)
    ck = R.Check(f"convex_upsample{'_3d' if taps == 27 else ''} {case} {T}x{H}x{W} t_halo={t_halo}")
    ck.add("out", out[:T * 2 * 16 * HW].view(T, 2, 4 * H, 4 * W), ref, R.tol_reduce(ref, f32, False))
    R.report(ck)
    assert (out[T * 2 * 16 * HW:] == R.SENTINEL).all(), "written past the output"


@pytest.mark.parametrize("case", S.CONVEX_LOGITS)
@pytest.mark.parametrize("BT,H,W", S.CONVEX_2D)
def test_convex_upsample_softmax(lib, BT, H, W, case):
    """ppms_convex_upsample against float64, tap by tap: logits of scale 30, one tap 80 above the rest, all taps equal, one tap at -1e4; a
    mask_ld beyond 144 with junk in the padding; H = 1 and W = 1 maps.  Tolerance: rule (c) of kernel_refs (8 x plain fp32 torch's error)."""
    _convex(case, BT, H, W, 9, 0, 7100)


@pytest.mark.parametrize("case", S.CONVEX_LOGITS)
@pytest.mark.parametrize("T,H,W,t_halo", S.CONVEX_3D)
def test_convex_upsample_3d_softmax(lib, T, H, W, t_halo, case):
    """ppms_convex_upsample_3d likewise over 27 taps, without and with a halo frame on either side of the T own frames"""
    _convex(case, T, H, W, 27, t_halo, 7200)
