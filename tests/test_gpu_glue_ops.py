"""GPU: the small glue kernels around the loop (glue_ops.hip, loop_ops.hip), each called through the C ABI and compared with the plain float64
reference of tests/kernel_refs.py.

Tolerances (kernel_refs.py states the rule; none comes from the code under test): (a) exact for copies, the relu half, flow_add and the hi
plane of any split; (b) 2e-5 * max(1, max|ref|) for split-bf16 outputs of elementwise math (resize-blend); (c) for reductions and
transcendentals (avgpool, the tanh half, the sigmoid) 8 x the max error of the same operation in plain fp32 torch on the CPU on the same
input.  axpby, fp32 elementwise: three roundings of at most 2^-24 relative to |a x| + |b y|, fused or not.  Every output buffer is
pre-filled with a sentinel (1.0); whatever lies outside what the kernel owns still holds it after the launch."""
import pytest
import torch

import kernel_refs as R
from kernel_refs import f32_in, f32_out, planes_are, report, sp_in, sp_out
from ppmstereo_amd.weights import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    return L


@pytest.mark.parametrize("case", R.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_flow_patch7(lib, case):
    """7 x 7 im2col of the 2-channel flow, windows that cross both borders at once: column tap 2 + c as F.unfold orders the taps, split as
    img_s2d splits (hi = bf16(x) exactly, |hi + lo - x| <= 2^-16 |x|), columns 98-127 zero"""
    L, lb = lib, lib.load()
    BT, H, W = case
    flow = R.flow_input(case)
    fd = flow.to(DEV)
    P = BT * H * W
    patch = sp_out(L, P, 136)
    L.check(lb.ppms_flow_patch7(fd.data_ptr(), patch.view(0, 128), BT, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    want = R.flow_patch(flow).reshape(P, 128)
    d = patch.own().cpu()
    report(R.split_check(R.Check(f"flow_patch7 {case}"), "planes", d[0, :, :98], d[1, :, :98], want[:, :98]))
    assert planes_are(patch, 98, 128, 0.0), "columns 98-127 must be zero"
    assert planes_are(patch, 128, 136, R.SENTINEL)


@pytest.mark.parametrize("case", R.UNC_CASES, ids=lambda c: "x".join(map(str, c)))
def test_unc_tail(lib, case):
    """sigmoid(w . x + b) against float64 (kind c), and partial[frame][blk] against the float64 block sums of the reference unc within
    256 x the unc tolerance + 255 2^-24 256 (the worst case of any-order fp32 summation of 256 terms <= 1)"""
    L, lb = lib, lib.load()
    BT, HW = case
    x, w, bias = R.unc_inputs(case)
    xs = sp_in(L, x.reshape(BT * HW, 128))
    wd = w.to(DEV)
    nblk = (HW + 255) // 256
    unc, part = f32_out(BT * HW), f32_out(BT * nblk)
    L.check(lb.ppms_unc_tail(xs.view(0, 128), wd.data_ptr(), bias, unc.data_ptr(), part.data_ptr(), BT, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    ref_unc, ref_part = R.unc_tail(x, w, bias)
    tol = R.tol_reduce(ref_unc, R.unc_tail_f32(x, w, bias), False)
    ck = R.Check(f"unc_tail {case}").add("unc", unc[:BT * HW].view(BT, HW), ref_unc, tol)
    report(ck.add("partial", part[:BT * nblk].view(BT, nblk), ref_part, R.unc_partial_tol(tol)))
    assert (unc[BT * HW:] == R.SENTINEL).all() and (part[BT * nblk:] == R.SENTINEL).all()


@pytest.mark.parametrize("ld", [4, 64])
def test_flow_add(lib, ld):
    """flow += dflow[:, :2]: the bits of torch's fp32 sum"""
    L, lb = lib, lib.load()
    P = 77
    flow, dflow = hash_normal((P, 2), 8000) * 4, hash_normal((P, 2), 8001)
    fd = f32_out(P * 2)
    fd[:P * 2] = flow.reshape(-1).to(DEV)
    dd = f32_in(dflow, ld)
    L.check(lb.ppms_flow_add(fd.data_ptr(), dd.data_ptr(), ld, P, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fd[:P * 2].view(P, 2).cpu(), flow + dflow)
    assert (fd[P * 2:] == R.SENTINEL).all()


@pytest.mark.parametrize("ab", R.RESIZE_AB, ids=["a0", "a.5"])
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sp_resize_blend(lib, case, ab):
    """a dst + b interp(src), bilinear, align_corners=True, on 16-channel views at channel 8 of 32-channel tensors (kind b).  With a = 0
    dst holds NaN before the launch: a = 0 must not read it."""
    L, lb = lib, lib.load()
    N, H, W, OH, OW = case
    a, b = ab
    dst0, src0 = R.resize_inputs(case)
    src = sp_in(L, src0.reshape(-1, 16), c0=8)
    dst = sp_in(L, dst0.reshape(-1, 16), c0=8)
    if a == 0.0:
        dst.data[:, :, 8:24] = float("nan")
    L.check(lb.ppms_sp_resize_blend(src.view(8, 16), dst.view(8, 16), N, H, W, OH, OW, a, b, L.stream_ptr()))
    torch.cuda.synchronize()
    ref = R.resize_blend(dst0, src0, OH, OW, a, b)
    report(R.Check(f"sp_resize_blend {case} a={a}").add("y", dst.to_f32(8, 16).reshape(N, OH, OW, 16), ref, R.tol_sp(ref)))
    assert planes_are(dst, 0, 8, R.SENTINEL) and planes_are(dst, 24, 32, R.SENTINEL)


@pytest.mark.parametrize("case", R.AVGPOOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_avgpool(lib, case):
    """k x k windows at stride k on 6 planes; output sizes floored as in F.avg_pool2d (9 x 14 at k = 4: the ragged border is left out)"""
    L, lb = lib, lib.load()
    k, H, W = case
    x = R.avgpool_input(case)
    xd = x.to(DEV)
    n = 6 * (H // k) * (W // k)
    out = f32_out(n)
    L.check(lb.ppms_avgpool(xd.data_ptr(), out.data_ptr(), 6, H, W, k, L.stream_ptr()))
    torch.cuda.synchronize()
    ref = R.avgpool(x, k)
    report(R.Check(f"avgpool {case}").add("y", out[:n].view(6, H // k, W // k), ref, R.tol_reduce(ref, R.avgpool_f32(x, k), False)))
    assert (out[n:] == R.SENTINEL).all()


@pytest.mark.parametrize("case", R.AXPBY_CASES, ids=lambda c: f"period{c[1]}")
def test_axpby(lib, case):
    """out = a x + b y[i mod period], in place (out == x) as the product calls it"""
    L, lb = lib, lib.load()
    n, period, a, b = case
    x, y = hash_normal((n,), 8100), hash_normal((period,), 8101)
    xd, yd = f32_out(n), y.to(DEV)
    xd[:n] = x.to(DEV)
    L.check(lb.ppms_axpby(xd.data_ptr(), yd.data_ptr(), xd.data_ptr(), a, b, period, n, L.stream_ptr()))
    torch.cuda.synchronize()
    report(R.Check(f"axpby period={period}").bound("out", xd[:n], R.axpby(x, y, a, b, period), R.axpby_tol(x, y, a, b, period)))
    assert (xd[n:] == R.SENTINEL).all()


def test_ctx_mix(lib):
    """net = tanh of the mean of the first 128 channels (kind c), inp = relu of the mean of the last 128 (exact: one fp32 sum, halved)"""
    L, lb = lib, lib.load()
    N, HW = 2, 35
    f, c = hash_normal((N, 256, HW), 8200), hash_normal((N, 256, HW), 8201)
    fd, cd = f.to(DEV), c.to(DEV)
    n = N * 128 * HW
    net, inp = f32_out(n), f32_out(n)
    L.check(lb.ppms_ctx_mix(fd.data_ptr(), cd.data_ptr(), net.data_ptr(), inp.data_ptr(), N, HW, L.stream_ptr()))
    torch.cuda.synchronize()
    ref_net, _ = R.ctx_mix(f, c)
    f32_net, f32_inp = R.ctx_mix_f32(f, c)                                      # inp: the fp32 sum, halved (exact), clamped -- the same bits
    ck = R.Check("ctx_mix").add("net", net[:n].view(N, 128, HW), ref_net, R.tol_reduce(ref_net, f32_net, False))
    report(ck.exact("inp", inp[:n].view(N, 128, HW), f32_inp))
    assert (net[n:] == R.SENTINEL).all() and (inp[n:] == R.SENTINEL).all()


@pytest.mark.parametrize("c0,c,src_ld", [(254, 2, 2), (0, 256, 260)], ids=["view254", "full"])
def test_f32_to_sp_and_back(lib, c0, c, src_ld):
    """ppms_f32_to_sp / ppms_sp_to_f32 on 37 pixels: the product's own odd call -- a 2-channel view at channel 254 of a 256-channel SP
    tensor, src_ld = 2 -- and the full 256 channels.  The split is exact in hi and within 2^-16 |x| in hi + lo; the way back is the fp32
    sum of the two planes, bit for bit; the neighbouring channels are untouched."""
    L, lb = lib, lib.load()
    P = 37
    x = hash_normal((P, c), 8300 + c) * 3
    xd = f32_in(x, src_ld)
    t = sp_out(L, P, 256)
    L.check(lb.ppms_f32_to_sp(xd.data_ptr(), src_ld, t.view(c0, c), P, L.stream_ptr()))
    torch.cuda.synchronize()
    d = t.own().cpu()
    ck = R.split_check(R.Check(f"f32_to_sp view({c0}, {c})"), "planes", d[0, :, c0:c0 + c], d[1, :, c0:c0 + c], x)
    assert planes_are(t, 0, c0, R.SENTINEL), "the neighbouring channels must not be written"
    back = f32_out(P * (c + 4))
    L.check(lb.ppms_sp_to_f32(t.view(c0, c), back.data_ptr(), c + 4, P, L.stream_ptr()))
    torch.cuda.synchronize()
    got = back[:P * (c + 4)].view(P, c + 4).cpu()
    ck.exact("sp_to_f32", got[:, :c], d[0, :, c0:c0 + c].float() + d[1, :, c0:c0 + c].float())
    report(ck.bound("round trip", got[:, :c], x, x.double().abs() * 2.0 ** -16))
    assert (got[:, c:] == R.SENTINEL).all() and (back[P * (c + 4):] == R.SENTINEL).all()
