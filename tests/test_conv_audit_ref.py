"""CPU: the descriptor-driven fp64 reference of tests/conv_audit.py checked against F.conv3d and the packers, and shown sensitive to the
mistakes it exists to catch (a missing sweep inverse, halo rows read as zeros, an extent one row too long).  Descriptors are built
with conv_desc + pack_for on CPU tensors and their pointers filled by hand; nothing is launched."""
import pytest
import torch
import torch.nn.functional as F

import conv_audit as A
from ppmstereo_amd import _lib as L
from ppmstereo_amd import packing as Pk
from ppmstereo_amd.convplan import CONV2, CONV2_SWEPT, CONV5, CONV6, GEMM1, STREAM, conv_desc, epilogue, pack_for
from ppmstereo_amd.weights import hash_normal

DEV = "cpu"


def _bf16_exact(w: torch.Tensor) -> torch.Tensor:
    """w rounded to bf16 (its pack then holds it exactly: the reference must match F.conv3d to float64 rounding)."""
    return w.to(torch.bfloat16).float()


def _kernel_of(layout):
    """pack key -> (ConvOp.version, ysweep)"""
    return (CONV2, True) if layout == CONV2_SWEPT else (layout, False)


# ------------------------------------------------------------------------------------------------ unpack round trip
UNPACK_CASES = [
    # layout, k3, segs, seg_pad, cout, cout_map, m
    (CONV2, (1, 3, 3), [64], None, 64, None, None),
    (CONV2, (3, 3, 3), [36], [64], 54, None, 128),
    (CONV2, (1, 3, 3), [320], None, 190, list(range(126)) + list(range(128, 192)), 192),
    (CONV2_SWEPT, (1, 5, 1), [64, 32], None, 64, None, None),
    (CONV2_SWEPT, (5, 1, 1), [64], None, 64, None, None),
    (CONV5, (1, 3, 3), [64], None, 192, None, 192),
    (CONV5, (1, 5, 1), [32, 64], None, 128, None, 128),
    (CONV5, (1, 1, 5), [64], None, 128, None, 128),
    (CONV5, (5, 1, 1), [64], None, 256, None, 256),
    (CONV6, (1, 3, 3), [64], None, 128, None, 128),
    (CONV6, (1, 5, 1), [64, 64], None, 128, None, 128),
    (CONV6, (1, 1, 15), [32], None, 64, None, 64),
    (CONV6, (3, 3, 3), [64], None, 190, list(range(126)) + list(range(128, 192)), 192),
    (GEMM1, (1, 1, 1), [98], [128], 128, None, 128),
    (GEMM1, (1, 1, 1), [48], [64], 96, None, 128),
    (STREAM, (1, 3, 3), [64], None, 64, None, 64),
    (STREAM, (5, 1, 1), [36, 92], [64, 128], 128, None, 128),
]


@pytest.mark.parametrize("layout,k3,segs,seg_pad,cout,cout_map,m", UNPACK_CASES)
def test_unpack_round_trip(layout, k3, segs, seg_pad, cout, cout_map, m):
    cin = sum(segs)
    w = hash_normal((cout, cin, *k3), 31)
    packed, bias, meta = pack_for(layout, w, None, segs, seg_pad, cout_map, m)
    pads = meta["seg_padded"]
    d = conv_desc([L.SP(None, None, p, p) for p in pads], (1, 1, 1), k3, epilogue(n_valid=1))
    d.M = meta["M"]
    version, ysweep = _kernel_of(layout)
    got = A.unpack_weights(version, ysweep, d, packed)                  # (M, Kpad, kt, kh, kw) float64
    want = torch.zeros(meta["M"], sum(pads), *k3, dtype=torch.float64)
    rows = torch.tensor(cout_map if cout_map is not None else list(range(cout)))
    src = dst = 0
    for c, p in zip(segs, pads):
        want[rows, dst:dst + c] = w[:, src:src + c].double()
        src, dst = src + c, dst + p
    err = (got - want).abs()
    assert (err <= want.abs() * 2.0 ** -16).all(), f"{layout} {k3}: max err {err.max().item():.3e}"


def test_unpack_round_trip_grouped():
    """conv_gemm6's grouped pack: rows [0, 128) are convolution 0 over its own segment, rows [128, 256) convolution 1 over its own."""
    ws = [hash_normal((128, 64, 1, 1, 5), 41 + i) for i in range(2)]
    packed, bias, meta = Pk.pack_conv6_grouped(ws, [None, None], 64)
    d = conv_desc([L.SP(None, None, 64, 64)] * 2, (1, 1, 1), (1, 1, 5), epilogue(n_valid=1))
    d.M, d.groups, d.m_split = 256, 2, 128
    got = A.unpack_weights(CONV6, False, d, packed)
    want = torch.cat([w.double() for w in ws], 0)
    assert ((got - want).abs() <= want.abs() * 2.0 ** -16).all()


# ------------------------------------------------------------------------------------------------ reference vs F.conv3d
def _epi_ref(kind, act, scale, v, aux=None, z=None, old=None):
    """include/ppms.h's epilogues, restated independently of conv_audit."""
    acts = {L.ACT_NONE: lambda x: x, L.ACT_RELU: F.relu, L.ACT_GELU: F.gelu, L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh,
            L.ACT_ELU1: lambda x: F.elu(x) + 1.0}
    if kind == L.EPI_STORE:
        return acts[act](v) * scale
    if kind == L.EPI_RESID:
        return acts[act](aux + v) * scale
    if kind == L.EPI_RH:
        return torch.sigmoid(v) * aux
    if kind == L.EPI_GRU:
        return (1 - z) * aux + z * torch.tanh(v)
    assert kind == L.EPI_ADDF32
    return old + v


class _Case:
    """A conv on CPU tensors: SP inputs with halo slabs, output buffers wider than the views, a hand-filled descriptor."""

    def __init__(self, layout, k3, segs, couts, T=2, H=5, W=7, th=0, halves=((L.EPI_STORE, L.ACT_NONE, 1.0),), out_c0=0, pre_off=None,
                 grouped=False, seed=5):
        self.k3, self.T, self.H, self.W, self.th, self.pre_off = k3, T, H, W, th, pre_off or 0
        self.version, self.ysweep = _kernel_of(layout)
        HW = H * W
        P = T * HW
        self.P = P
        self.xs = [L.SPTensor(P, c + 32, DEV, before=th * HW, after=th * HW) for c in segs]      # 32 channels beyond each view
        seg_views = [x.view(0, c) for x, c in zip(self.xs, segs)]
        cin = segs[0] if grouped else sum(segs)
        self.ws = [_bf16_exact(hash_normal((co, cin, *k3), seed + i) / (cin * k3[0] * k3[1] * k3[2]) ** 0.5) for i, co in enumerate(couts)]
        self.bs = [_bf16_exact(hash_normal((co,), seed + 10 + i)) for i, co in enumerate(couts)]
        if grouped:
            packed, bias, meta = Pk.pack_conv6_grouped(self.ws, self.bs, cin)
            m_split = 128
        else:
            m_split = 64 * ((couts[0] + 63) // 64) if len(couts) == 2 else 0
            w = torch.cat(self.ws, 0)
            cmap = list(range(couts[0])) + (list(range(m_split, m_split + couts[1])) if len(couts) == 2 else [])
            M = m_split + 64 * ((couts[1] + 63) // 64) if len(couts) == 2 else None
            if layout in (CONV5, CONV6) and M is None:
                M = 128 if couts[0] <= 128 else 256
            packed, bias, meta = pack_for(layout, w, torch.cat(self.bs), segs, None, cmap, M)
        self.keep = [packed, bias]
        self.outs, epis = [], []
        for h, (kind, act, scale) in enumerate(halves):
            co = couts[h]
            osp = L.SPTensor(P, out_c0 + co + 16, DEV)
            of = torch.zeros(P, co + 8)
            aux = L.SPTensor(P, co + 8, DEV)
            z = torch.zeros(P, co + 4)
            pre = torch.zeros(P, co + (pre_off or 0) + 4) if pre_off is not None else None
            kw = dict(kind=kind, act=act, scale=scale, n_valid=co, out_f32=of, out_f32_ld=of.shape[1])
            if kind != L.EPI_ADDF32:
                kw["out_sp"] = osp.view(out_c0, co)
            if kind in (L.EPI_RESID, L.EPI_RH, L.EPI_GRU):
                kw["aux_sp"] = aux.view(4, co)
            if kind == L.EPI_GRU:
                kw.update(aux_f32=z, aux_f32_ld=z.shape[1])
            if pre is not None:
                kw.update(pre_f32=pre, pre_off=pre_off)
            epis.append(epilogue(**kw))
            self.outs.append(dict(osp=osp, of=of, aux=aux, z=z, pre=pre, kind=kind, act=act, scale=scale, co=co))
        d = conv_desc(seg_views, (T, H, W), k3, epis[0], epis[1] if len(epis) > 1 else None, m_split, th, 0)
        d.w, d.bias, d.M = packed.data_ptr(), bias.data_ptr(), meta["M"]
        if d.m_split == 0:
            d.m_split = meta["M"]
        if grouped:
            d.groups = 2
        self.d, self.segs, self.grouped = d, segs, grouped

    def run_reference(self, **kw):
        self.pool = A.Pool(self)
        rs, errs = A.bind_regions(self.d, self.pool)
        assert not errs, errs
        A.fill_storages(self.pool, rs, self.d, seed=3)
        pix = torch.arange(self.P)
        return rs, A.reference(self.d, self.version, self.ysweep, self.pool, rs, pix, **kw)

    def conv3d(self):
        """F.conv3d in float64 over the own frames and the halo slabs (frames beyond them: zero padding), per epilogue half."""
        T, H, W, th, k3 = self.T, self.H, self.W, self.th, self.k3
        xs = [x.data[0, :, :c].double() + x.data[1, :, :c].double() for x, c in zip(self.xs, self.segs)]
        vol = lambda x: x.reshape(1, T + 2 * th, H, W, -1).permute(0, 4, 1, 2, 3)
        res = []
        for h, (w, b) in enumerate(zip(self.ws, self.bs)):
            x = xs[h] if self.grouped else torch.cat(xs, 1)
            y = F.conv3d(vol(x), w.double(), b.double(), padding=tuple(k // 2 for k in k3))[:, :, th:th + T]
            res.append(y.permute(0, 2, 3, 4, 1).reshape(T * H * W, -1))
        return res

    def expected(self, h, v):
        o = self.outs[h]
        co = o["co"]
        if o["pre"] is not None:
            v = v + o["pre"][:, self.pre_off:self.pre_off + co].double()
        aux = o["aux"].data[0, :, 4:4 + co].double() + o["aux"].data[1, :, 4:4 + co].double()
        return _epi_ref(o["kind"], o["act"], o["scale"], v, aux, o["z"][:, :co].double(), o["of"][:, :co].double())


def _check(case, rs, exp, tol=1e-11):
    got = case.conv3d()
    for h in range(len(case.outs)):
        want = case.expected(h, got[h])
        for name in (f"epi[{h}].out_sp", f"epi[{h}].out_f32"):
            if name in exp:
                err = (exp[name] - want).abs().max().item()
                assert err <= tol * max(1.0, want.abs().max().item()), f"{name}: {err:.3e}"


REF_CASES = [
    # id, layout, k3, segs, couts, kwargs
    ("store_none", CONV2, (1, 3, 3), [64], [64], {}),
    ("store_relu_scale", GEMM1, (1, 1, 1), [64, 32], [96], dict(halves=((L.EPI_STORE, L.ACT_RELU, 0.25),))),
    ("store_gelu", CONV5, (1, 3, 3), [32], [128], dict(halves=((L.EPI_STORE, L.ACT_GELU, 1.0),))),
    ("store_sigmoid", STREAM, (1, 5, 1), [64], [64], dict(halves=((L.EPI_STORE, L.ACT_SIGMOID, 1.0),))),
    ("store_tanh", CONV6, (1, 1, 5), [32, 32], [128], dict(halves=((L.EPI_STORE, L.ACT_TANH, 1.0),))),
    ("store_elu1", CONV2_SWEPT, (1, 5, 1), [64], [64], dict(halves=((L.EPI_STORE, L.ACT_ELU1, 0.5),))),
    ("resid_relu", CONV2, (1, 1, 1), [32], [64], dict(halves=((L.EPI_RESID, L.ACT_RELU, 1.0),))),
    ("rh", CONV6, (1, 5, 1), [64], [128], dict(halves=((L.EPI_RH, L.ACT_NONE, 1.0),))),
    ("gru", CONV5, (5, 1, 1), [64], [128], dict(halves=((L.EPI_GRU, L.ACT_NONE, 1.0),), T=6)),
    ("addf32", CONV2, (1, 3, 3), [32], [64], dict(halves=((L.EPI_ADDF32, L.ACT_NONE, 1.0),))),
    ("two_halves", CONV2, (1, 1, 15), [64], [64, 54], dict(halves=((L.EPI_STORE, L.ACT_SIGMOID, 1.0), (L.EPI_RH, L.ACT_NONE, 1.0)), W=19)),
    ("two_halves_gemm6", CONV6, (1, 3, 3), [64], [126, 64], dict(halves=((L.EPI_STORE, L.ACT_RELU, 1.0), (L.EPI_STORE, L.ACT_RELU, 1.0)))),
    ("grouped", CONV6, (1, 1, 5), [64, 64], [128, 128], dict(grouped=True, halves=((L.EPI_STORE, L.ACT_SIGMOID, 1.0), (L.EPI_RH, L.ACT_NONE, 1.0)))),
    ("halo1_3x3x3", CONV6, (3, 3, 3), [64], [128], dict(th=1, T=3)),
    ("halo2_5x1x1", CONV5, (5, 1, 1), [64, 32], [128], dict(th=2, T=3, halves=((L.EPI_GRU, L.ACT_NONE, 1.0),))),
    ("halo2_stream", STREAM, (5, 1, 1), [64], [64], dict(th=2, T=2)),
    ("pre_offset", CONV2, (1, 1, 15), [32], [64, 64], dict(pre_off=64, halves=((L.EPI_STORE, L.ACT_GELU, 1.0), (L.EPI_RH, L.ACT_NONE, 1.0)), W=17)),
    ("out_view_offset", CONV6, (1, 3, 3), [32], [64], dict(out_c0=256)),
]


@pytest.mark.parametrize("cid,layout,k3,segs,couts,kw", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_reference_vs_conv3d(cid, layout, k3, segs, couts, kw):
    case = _Case(layout, k3, segs, couts, **kw)
    rs, exp = case.run_reference()
    assert {n for n in exp} >= {f"epi[{h}].out_f32" for h in range(len(couts))}
    _check(case, rs, exp)


def test_reference_misses_without_sweep_inverse():
    """A y-swept and a 2-D swept pack read in natural tap order (two 32-channel chunks: the orders differ) must not pass."""
    for layout, k3 in ((CONV6, (1, 5, 1)), (CONV5, (1, 3, 3)), (CONV2_SWEPT, (3, 3, 1))):
        case = _Case(layout, k3, [64], [128] if layout != CONV2_SWEPT else [64])
        rs, exp = case.run_reference()
        _check(case, rs, exp)
        _, bad = case.run_reference(sweep_inverse=False)
        with pytest.raises(AssertionError):
            _check(case, rs, bad)


def test_reference_misses_halo_as_zeros():
    case = _Case(CONV5, (5, 1, 1), [64], [128], th=2, T=3)
    rs, exp = case.run_reference()
    _check(case, rs, exp)
    _, bad = case.run_reference(halo_zero=True)
    with pytest.raises(AssertionError):
        _check(case, rs, bad)


def test_resolver_rejects_extent_one_row_too_long():
    case = _Case(CONV2, (1, 3, 3), [32], [64])
    pool = A.Pool(case)
    _, errs = A.bind_regions(case.d, pool)
    assert not errs, errs
    short = torch.zeros(case.P - 1, 72)                  # one pixel row short of the launch's own rows
    case.keep.append(short)
    case.d.epi[0].out_f32, case.d.epi[0].out_f32_ld = short.data_ptr(), 72
    _, errs = A.bind_regions(case.d, A.Pool(case))
    assert any("epi[0].out_f32" in e and "outside" in e for e in errs), errs
    # input rows: a descriptor that claims one halo frame its segment does not have
    case2 = _Case(CONV5, (3, 1, 1), [64], [128])
    case2.d.t_halo = 1
    _, errs = A.bind_regions(case2.d, A.Pool(case2))
    assert any(e.startswith("seg[0].hi") and "outside" in e for e in errs), errs
    # a pointer into no tensor of the owners
    case3 = _Case(CONV2, (1, 3, 3), [32], [64])
    stray = torch.zeros(case3.P, 64)
    case3.d.epi[0].out_f32, case3.d.epi[0].out_f32_ld = stray.data_ptr(), 64
    _, errs = A.bind_regions(case3.d, A.Pool(case3))
    assert any("lies in no live tensor" in e for e in errs), errs


def test_overlap_detection():
    """An output view that shares channels with an input view of the same buffer is a read/write overlap; adjacent channels are not."""
    case = _Case(CONV2, (1, 1, 1), [64], [64])
    x = case.xs[0]
    case.d.epi[0].out_sp = x.view(64, 32)               # channels 64..95 of a 96-channel buffer whose view reads 0..63: adjacent
    case.d.epi[0].n_valid = 32
    _, errs = A.bind_regions(case.d, A.Pool(case))
    assert not errs, errs
    case.d.epi[0].out_sp = x.view(48, 32)               # channels 48..79: overlaps the read channels 48..63
    _, errs = A.bind_regions(case.d, A.Pool(case))
    assert any("overlaps input seg[0]" in e for e in errs), errs


def test_pixel_sample_covers_edges():
    pix = A.pixel_sample(40, 184, 320, 0, "cpu")
    T, H, W = 40, 184, 320
    n = T * H * W
    s = set(pix.tolist())
    assert n - 1 in s and all(p in s for p in range(n - 4096, n))
    for t in (0, 1, 20, 38, 39):
        for y in (0, 1, 2, 92, 181, 182, 183):
            assert all((t * H + y) * W + x in s for x in range(W))
        for x in (0, 1, 160, 318, 319):
            assert all((t * H + y) * W + x in s for y in range(H))
    assert A.pixel_sample(5, 80, 128, 0, "cpu").numel() == 5 * 80 * 128


def test_sp_split_check():
    """The SP-representation check accepts the split every epilogue writes (ties from lo's rounding included) and rejects a truncated hi
    or a lo plane from another element."""
    x = hash_normal((1 << 16,), 77) * 3
    hi, lo = Pk.split_bf16(x)
    assert A.sp_split_violations(hi, lo) == 0
    r = (hi.float() + lo.float()).to(torch.bfloat16)
    assert (r != hi).any(), "the sample must contain the ties the check allows"
    trunc = (x.view(torch.int32) & ~0xFFFF).view(torch.float32)            # hi truncated instead of rounded
    hi_t = trunc.to(torch.bfloat16)
    assert A.sp_split_violations(hi_t, (x - hi_t.float()).to(torch.bfloat16)) > 1000
    assert A.sp_split_violations(hi, lo.roll(1) * 300) > 1000
