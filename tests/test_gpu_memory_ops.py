"""GPU: the pick-and-play memory read-out -- frame similarity (ppms_qk_pool / _cos / _similarity), the QAM pick (ppms_qam_select and the
merged ppms_pick_prep_k), the attention operands (ppms_attn_prep_q / _k) and the read-out itself (ppms_mem_attn: the 32-query kernel with
and without a workspace, the 64-query kernel with every tile count, frames-per-workgroup value and idle-wave shape, the sharded form and
the fix-up pass) -- each called through the C ABI and compared with the plain float64 reference of tests/kernel_refs.py.

Tolerances: kernel_refs.py states the rule; none comes from the code under test.  SEL and the usage counter are exact, the operands are
bit-exact (one fp32 operation rounded to bf16; the build does not contract the multiply-add), the read-out keeps the per-element bound
tests/test_gpu_ops.py derives.  Every output holds a sentinel before the launch, the attention workspace holds NaN bit patterns, and a
refused call is shown to launch nothing."""
import ctypes as C

import pytest
import torch

import kernel_refs as R
from kernel_refs import f32_in, f32_out, planes_are, report, sp_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16 = torch.bfloat16
PAT = 0x7B7B                                                               # bit pattern of untouched bf16 operand buffers


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    return L


def bf16_out(n, guard=512):
    t = torch.empty(n + guard, dtype=BF16, device=DEV)
    t.view(torch.int16).fill_(PAT)
    return t


def untouched(t):
    return bool((t.view(torch.int16) == PAT).all().item())


def same_bits(a, b):
    """bit equality of two bf16 tensors of values, NaN == NaN (payloads are not compared across devices)"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()) and \
        bool((torch.signbit(a) == torch.signbit(b))[~torch.isnan(a)].all())


def refused(L, rc, message):
    assert rc == -1, f"PPMS_EINVAL expected, got {rc}"
    with pytest.raises(RuntimeError, match=message):
        L.check(rc)


# ------------------------------------------------------------------------------------------------ frame similarity
@pytest.mark.parametrize("ld", [128, 256])
@pytest.mark.parametrize("data", R.SIM_DATA)
@pytest.mark.parametrize("case", R.SIM_CASES, ids=lambda c: "T%dH%dW%d" % c)
def test_qk_similarity(lib, case, data, ld):
    """ppms_qk_similarity on the first T frames; then the sharded window's way: ppms_qk_pool per "rank" (frames [0, T) and the other
    three), the descriptors assembled into one table of Tg = T + 3 frames, ppms_qk_cos on it -- against float64, and bit-identical to
    ppms_qk_similarity on the T frames and on all Tg.  ld = 256: q | k in one row, as the engine lays them out.  "edge": a constant-zero
    frame (norm 0, the eps branch: finite, 0) and a frame x 1e-6."""
    L, lb, s = lib, lib.load(), lib.stream_ptr()
    T, H, W = case
    Tg, HW, cells = T + R.SIM_EXTRA, H * W, (H // 4) * (W // 4)
    q, k = R.sim_inputs(case, data)
    if ld == 256:
        buf = torch.cat([q, k], -1).reshape(Tg * HW, 256).contiguous().to(DEV)
        qp, kp = buf.data_ptr(), buf.data_ptr() + 512
    else:
        qd, kd = q.reshape(Tg * HW, 128).contiguous().to(DEV), k.reshape(Tg * HW, 128).contiguous().to(DEV)
        qp, kp = qd.data_ptr(), kd.data_ptr()
    pooled, sim = f32_out(2 * T * cells), f32_out(T * T)
    L.check(lb.ppms_qk_similarity(qp, kp, ld, pooled.data_ptr(), sim.data_ptr(), T, H, W, s))
    pa, pb = f32_out(2 * T * cells), f32_out(2 * R.SIM_EXTRA * cells)
    L.check(lb.ppms_qk_pool(qp, kp, ld, pa.data_ptr(), T, H, W, s))
    L.check(lb.ppms_qk_pool(qp + T * HW * ld * 4, kp + T * HW * ld * 4, ld, pb.data_ptr(), R.SIM_EXTRA, H, W, s))
    torch.cuda.synchronize()
    table = torch.cat([pa[:2 * T * cells].view(2, T, cells), pb[:2 * R.SIM_EXTRA * cells].view(2, R.SIM_EXTRA, cells)], 1).contiguous()
    simg, pall, simall = f32_out(Tg * Tg), f32_out(2 * Tg * cells), f32_out(Tg * Tg)
    L.check(lb.ppms_qk_cos(table.data_ptr(), simg.data_ptr(), Tg, cells, s))
    L.check(lb.ppms_qk_similarity(qp, kp, ld, pall.data_ptr(), simall.data_ptr(), Tg, H, W, s))
    torch.cuda.synchronize()
    report(R.sim_check(case, data, T, sim[:T * T].view(T, T), pooled[:2 * T * cells].view(2, T, cells), f"qk_similarity {case} {data} ld={ld}"))
    report(R.sim_check(case, data, Tg, simg[:Tg * Tg].view(Tg, Tg), table, f"qk_pool + qk_cos {case} {data} ld={ld} Tg={Tg}"))
    assert torch.equal(pa, pooled), "ppms_qk_pool != the pooling of ppms_qk_similarity"
    assert torch.equal(simg[:Tg * Tg].view(Tg, Tg)[:T, :T], sim[:T * T].view(T, T)), "qk_cos on the gathered table != qk_similarity on this rank's frames"
    assert torch.equal(simg, simall) and torch.equal(pall[:2 * Tg * cells].view(2, Tg, cells), table), "the two halves != ppms_qk_similarity on all frames"
    for t, n in ((pooled, 2 * T * cells), (sim, T * T), (pb, 2 * R.SIM_EXTRA * cells), (simg, Tg * Tg)):
        assert (t[n:] == R.SENTINEL).all(), "written past the output"


# ------------------------------------------------------------------------------------------------ QAM pick
PICK_N, PICK_LD = 3, 136                                                   # key pixels of the merged launch; ld with 8 junk columns


def _pick_buffers(T):
    sel = torch.full((T * 5 + 8,), -1, dtype=torch.int32, device=DEV)
    return sel, f32_out(T * 5), f32_out(T * T)


def _pick_outputs(T, sel, shat, score):
    assert (sel[T * 5:] == -1).all() and (shat[T * 5:] == R.SENTINEL).all() and (score[T * T:] == R.SENTINEL).all(), "written past an output"
    return score[:T * T].view(T, T), sel[:T * 5].view(T, 5), shat[:T * 5].view(T, 5)


def _pick_both(L, T, sim, strive, part, nblk, HW, key, pe):
    """one pick from `strive` (T, T) on both entry points -> [(score, sel, shat, new counter)] x 2, K' of the merged launch (with guard)"""
    lb, s = L.load(), L.stream_ptr()
    ksel = min(5, T)
    simd, partd = sim.to(DEV).contiguous(), part.to(DEV).contiguous()
    st_sel, st_in, st_out = strive.float().to(DEV).contiguous(), strive.float().to(DEV).contiguous(), torch.full((T * T + 8,), -7.0, device=DEV)
    a, b = _pick_buffers(T), _pick_buffers(T)
    kb = bf16_out(T * ksel * PICK_N * 128)
    L.check(lb.ppms_qam_select(simd.data_ptr(), st_sel.data_ptr(), partd.data_ptr(), nblk, HW, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), T, s))
    L.check(lb.ppms_pick_prep_k(simd.data_ptr(), st_in.data_ptr(), st_out.data_ptr(), partd.data_ptr(), nblk, HW, b[0].data_ptr(), b[1].data_ptr(),
                                b[2].data_ptr(), key.data_ptr(), PICK_LD, pe.data_ptr(), kb.data_ptr(), T, PICK_N, s))
    torch.cuda.synchronize()
    assert torch.equal(st_in.cpu(), strive.float()) and (st_out[T * T:] == -7.0).all(), "pick_prep_k: the input counter or the tail of the output"
    return [(*_pick_outputs(T, *a), st_sel), (*_pick_outputs(T, *b), st_out[:T * T].view(T, T))], kb


def _check_kprime(T, kb, key, pe, sel, shat):
    """K' of the merged launch, bit for bit bf16(key * shat + pe) in fp32 torch from the s_hat the kernel itself returned (its picks are
    checked against the reference by the caller); the guard rows behind the last [clip][slot] untouched"""
    ksel, n = min(5, T), PICK_N
    want = R.prep_k(key[:, :128].cpu().reshape(T, n, 128), pe.cpu(), sel.cpu(), shat.cpu(), ksel)
    assert same_bits(kb[:T * ksel * n * 128].view(T, ksel, n, 128), want), "K' != bf16(key * s_hat + pe)"
    assert untouched(kb[T * ksel * n * 128:]), "a write behind the last [clip][slot]"


@pytest.mark.parametrize("T", list(R.PICK_CASES))
def test_qam_pick(lib, T):
    """six consecutive picks with the evolving usage counter on ppms_qam_select and on ppms_pick_prep_k, each against the float64 restatement
    of ppmstereo.py:501-513, 532-533: SEL and the counter exactly, SCORE and SHAT by the reduction rule.  T > 8: the second group of eight
    confidence sums; nblk > 64: a lane's second block; T = 64: the documented maximum.  No row of these cases is a near tie (the CPU test
    asserts a gap of 256 x the fp32 error).  T = 1: NaN similarities, as the product has them -- frame 0 is picked, the counter counts."""
    L = lib
    nblk = R.PICK_CASES[T]
    sim, parts, HW = R.pick_inputs(T)
    key = f32_in(R.hash_normal((T * PICK_N, 128), 9700 + T), PICK_LD)
    pe = torch.sin(R.hash_normal((T, 128), 9701 + T) * 3.0).float().to(DEV)
    cks = [R.Check(f"qam_select T={T} nblk={nblk}"), R.Check(f"pick_prep_k T={T} nblk={nblk}")]
    strive = torch.ones(T, T)
    for it, part in enumerate(parts):
        res, kb = _pick_both(L, T, sim, strive, part, nblk, HW, key, pe)
        for ck, (score, sel, shat, new) in zip(cks, res):
            R.pick_check(T, it, score, sel, shat, new, ck=ck)
        _check_kprime(T, kb, key, pe, res[1][1], res[1][2])
        strive = res[0][3].cpu()
    for ck in cks:
        report(ck)


@pytest.mark.parametrize("name", list(R.PICK_TIES))
def test_qam_pick_exact_ties_go_to_the_lowest_index(lib, name):
    """two or three bit-equal score columns (equal similarity and counter columns, equal block sums) that straddle the 5th / 6th rank in every
    row: both entry points pick the lowest frame indices of the tie (include/ppms.h)"""
    L = lib
    T, tied, first, picked = R.PICK_TIES[name]
    sim, strive, part = R.tie_inputs(name)
    key = f32_in(R.hash_normal((T * PICK_N, 128), 9710 + T), PICK_LD)
    pe = torch.sin(R.hash_normal((T, 128), 9711 + T) * 3.0).float().to(DEV)
    res, kb = _pick_both(L, T, sim, strive, part, R.TIE_NBLK, R.TIE_HW, key, pe)
    for entry, (score, sel, shat, new) in zip(("qam_select", "pick_prep_k"), res):
        assert all(torch.equal(score[:, t], score[:, tied[0]]) for t in tied), "the tied columns are not bit-equal on the device"
        assert sel.cpu().tolist() == [list(picked)] * T, (entry, sel.cpu().tolist())
        report(R.tie_check(name, score, sel, shat, new, f"{entry} tie {name}"))
    _check_kprime(T, kb, key, pe, res[1][1], res[1][2])


# ------------------------------------------------------------------------------------------------ attention operands
@pytest.mark.parametrize("ld", R.PREP_LD)
@pytest.mark.parametrize("n", R.PREP_N)
def test_attn_prep(lib, n, ld):
    """ppms_attn_prep_q / _k bit for bit bf16(q + pe) and bf16(key * s_hat + pe), each one fp32 operation per step: the whole window (7
    frames); then the sharded form -- T = 2 clips of this rank, q and pe offset to its first frame, sel rows that index all 7 frames --
    with ksel 1, 3 and 5"""
    L, lb, s = lib, lib.load(), lib.stream_ptr()
    T, Tg = R.PREP_T, R.PREP_TG
    q, key, pe, sel, shat = R.prep_inputs(n)
    if ld == 256:
        buf = torch.cat([q, key], -1).reshape(Tg * n, 256).contiguous().to(DEV)
        qp, kp = buf.data_ptr(), buf.data_ptr() + 512
    else:
        qd, kd = q.reshape(Tg * n, 128).contiguous().to(DEV), key.reshape(Tg * n, 128).contiguous().to(DEV)
        qp, kp = qd.data_ptr(), kd.data_ptr()
    ped, seld, shatd = pe.to(DEV), sel.to(DEV), shat.to(DEV)
    qb = bf16_out(Tg * n * 128)
    L.check(lb.ppms_attn_prep_q(qp, ld, ped.data_ptr(), qb.data_ptr(), Tg, n, s))
    torch.cuda.synchronize()
    assert torch.equal(qb[:Tg * n * 128].view(Tg, n, 128).cpu(), R.prep_q(q, pe)) and untouched(qb[Tg * n * 128:])
    f0 = 3                                                                  # this rank's first frame
    qb = bf16_out(T * n * 128)
    L.check(lb.ppms_attn_prep_q(qp + f0 * n * ld * 4, ld, ped.data_ptr() + f0 * 512, qb.data_ptr(), T, n, s))
    torch.cuda.synchronize()
    assert torch.equal(qb[:T * n * 128].view(T, n, 128).cpu(), R.prep_q(q[f0:f0 + T], pe[f0:f0 + T])) and untouched(qb[T * n * 128:])
    for ksel in R.PREP_KSEL:
        kb = bf16_out(T * ksel * n * 128)
        L.check(lb.ppms_attn_prep_k(kp, ld, ped.data_ptr(), seld.data_ptr(), shatd.data_ptr(), kb.data_ptr(), T, ksel, n, s))
        torch.cuda.synchronize()
        assert torch.equal(kb[:T * ksel * n * 128].view(T, ksel, n, 128).cpu(), R.prep_k(key, pe, sel, shat, ksel)), ksel
        assert untouched(kb[T * ksel * n * 128:]), "a write behind the last [clip][slot]"


def test_attn_prep_refuses_misaligned_or_empty_operands(lib):
    """the operand kernels load q / key / pe as f32x4 and store bf16x8: a pointer that is not 16-byte aligned, T <= 0 or n <= 0 is
    refused with PPMS_EINVAL and its own message before any launch (no output byte changes)"""
    L, lb, s = lib, lib.load(), lib.stream_ptr()
    T, n = 2, 5
    q, key, pe, sel, shat = R.prep_inputs(n)
    good = f32_in(q[:T].reshape(T * n, 128), 128)
    bad = f32_in(q[:T].reshape(T * n, 128), 128, misaligned=True)
    ped = torch.zeros(T * 128 + 4, device=DEV)
    seld, shatd = sel.to(DEV), shat.to(DEV)
    out = bf16_out(T * 5 * n * 128)
    sim, st0, st1, part = torch.zeros(T, T, device=DEV), torch.ones(T, T, device=DEV), f32_out(T * T), torch.ones(T, 1, device=DEV)
    psel, pshat = torch.full((T * 5,), -1, dtype=torch.int32, device=DEV), f32_out(T * 5)
    g, b, p, pm, o, om = good.data_ptr(), bad.data_ptr(), ped.data_ptr(), ped.data_ptr() + 4, out.data_ptr(), out.data_ptr() + 8
    assert b % 16 == 4 and pm % 16 == 4 and om % 16 == 8
    for args in ((b, 128, p, o, T, n), (g, 128, pm, o, T, n), (g, 128, p, om, T, n)):
        refused(L, lb.ppms_attn_prep_q(*args, s), "attn_prep_q: .*16-byte aligned")
    for args in ((g, 128, p, o, 0, n), (g, 128, p, o, T, 0), (g, 128, p, o, T, -1)):
        refused(L, lb.ppms_attn_prep_q(*args, s), "attn_prep_q: bad arguments")
    sd, hd = seld.data_ptr(), shatd.data_ptr()
    for args in ((b, 128, p, sd, hd, o, T, 5, n), (g, 128, pm, sd, hd, o, T, 5, n), (g, 128, p, sd, hd, om, T, 5, n)):
        refused(L, lb.ppms_attn_prep_k(*args, s), "attn_prep_k: .*16-byte aligned")
    for args in ((g, 128, p, sd, hd, o, 0, 5, n), (g, 128, p, sd, hd, o, T, 5, 0)):
        refused(L, lb.ppms_attn_prep_k(*args, s), "attn_prep_k: bad arguments")
    head = (sim.data_ptr(), st0.data_ptr(), st1.data_ptr(), part.data_ptr(), 1, n, psel.data_ptr(), pshat.data_ptr(), None)
    for args in ((b, 128, p, o), (g, 128, pm, o), (g, 128, p, om)):
        refused(L, lb.ppms_pick_prep_k(*head, *args, T, n, s), "pick_prep_k: .*16-byte aligned")
    torch.cuda.synchronize()
    assert untouched(out) and (st1 == R.SENTINEL).all() and (psel == -1).all() and (pshat == R.SENTINEL).all(), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------ memory attention
XC, MF0, MFG0 = 272, 8, 136                                                # channels of the mf | mfg tensor; first channel of either view


class _Attn:
    """the device operands of named inputs (kernel_refs.attn_named_inputs), shared by the formats and launch forms of a case"""

    def __init__(self, L, name):
        (q, k, v, sel, ksel, mf), self.scale = R.attn_named_inputs(*name)
        self.L, self.name, self.ksel, self.mf, self.v = L, name, ksel, mf, v
        self.T, self.n = q.shape[:2]
        self.qb, self.kb, self.sel = q.to(BF16).to(DEV), k.to(BF16).to(DEV), sel.to(DEV)
        assert torch.equal(self.qb.float().cpu(), q) and torch.equal(self.kb.float().cpu(), k), "the reference must see what the kernel sees"
        self.beta = torch.tensor([R.ATTN_BETA], device=DEV)
        self.vt = {}

    def vt_for(self, p_format):
        if p_format not in self.vt:
            self.vt[p_format] = self.L.vt_image(self.v, p_format).to(DEV)
            assert torch.equal(self.L.vt_values(self.vt[p_format], p_format).cpu(), self.v)
        return self.vt[p_format]

    def workspace(self):
        """(float32 view of the workspace filled with NaN bit patterns, 4 words of guard behind it)"""
        nbytes = int(self.L.load().ppms_mem_attn_workspace_bytes(self.T, self.ksel, self.n))
        assert nbytes % 4 == 0
        return torch.full((nbytes // 4 + 4,), NAN, device=DEV)

    def run(self, p_format, ws, frames, with_mf=True):
        """-> raw (T, n, 128) bf16, the mf | mfg tensor"""
        L, T, n = self.L, self.T, self.n
        X = sp_out(L, T * n, XC)
        X.set_f32(self.mf.to(DEV), MF0)
        raw = bf16_out(T * n * 128)
        mfv = X.view(MF0, 128) if with_mf else L.SP(None, None, 0, 0)
        L.check(L.load().ppms_mem_attn(self.qb.data_ptr(), self.kb.data_ptr(), self.vt_for(p_format).data_ptr(), self.sel.data_ptr(), self.ksel, self.scale,
                                       self.beta.data_ptr(), mfv, X.view(MFG0, 128), raw.data_ptr(), T, n, L.ptr(ws), frames, p_format, L.stream_ptr()))
        torch.cuda.synchronize()
        assert untouched(raw[T * n * 128:]), "written past out_bf16"
        assert planes_are(X, 0, MF0, R.SENTINEL) and planes_are(X, MFG0 + 128, XC, R.SENTINEL), "columns outside the views must keep the sentinel"
        assert torch.equal(X.to_f32(MF0, 128).cpu(), self.mf), "mf was written"
        return raw[:T * n * 128].view(T, n, 128), X

    def check(self, p_format, ws, frames, label):
        """one call against the reference, then the mf.hi == NULL form of the same call: hi plane = the raw output bit for bit, lo plane 0"""
        raw, X = self.run(p_format, ws, frames)
        ck = R.attn_check(self.name, p_format, raw, X.to_f32(MFG0, 128), label)
        raw2, X2 = self.run(p_format, ws, frames, with_mf=False)
        hi, lo = X2.own()[0, :, MFG0:MFG0 + 128], X2.own()[1, :, MFG0:MFG0 + 128]
        assert torch.equal(raw2.view(torch.int16), raw.view(torch.int16)), "the read-out depends on the aggregation form"
        assert torch.equal(hi.reshape(raw.shape).view(torch.int16), raw.view(torch.int16)) and (lo.view(torch.int16) == 0).all(), "mf.hi == NULL: hi = hid, lo = 0"
        return ck

    def partials(self, ws, nsp):
        """(O rows, (m, l) rows) the combine reads: nsp partial sets per clip"""
        T, n, ksel = self.T, self.n, self.ksel
        return ws[:T * nsp * n * 128], ws[T * ksel * n * 128:T * ksel * n * 128 + T * nsp * n * 2]

    def flags(self, ws, nsp):
        """[clip][split][256-query block][2] int32"""
        T, n, g = self.T, self.n, (self.n + 255) // 256
        off = T * self.ksel * n * 130
        return ws.view(torch.int32)[off:off + T * nsp * g * 2].view(T, nsp, g, 2), ws.view(torch.int32)[off + T * nsp * g * 2:-4]


P_FORMATS = [pytest.param(1, id="p_fp16"), pytest.param(0, id="p_bf16")]
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()


@pytest.mark.parametrize("ksel", R.ATTN32_KSEL)
@pytest.mark.parametrize("n", R.ATTN32_N)
def test_mem_attn_32_query_kernel(lib, n, ksel):
    """maps of fewer than 32, 64 and 128 queries (the 1/16 scale of small inputs), n % 8 != 0 (element-wise V loads) and n = 72 (vector rows,
    a partial tile): the fused launch (no workspace) and, with a workspace, the per-frame split + combine; both p_formats; T = 2 clips over
    max(2, ksel + 1) frames of vt"""
    a = _Attn(lib, ("table", 32, n, ksel))
    assert lib.load().ppms_mem_attn_splits(a.T, ksel, n, 0) == 0, "n % 64 != 0: not the 64-query kernel"
    for p in (1, 0):
        report(a.check(p, None, 0, f"mem_attn32 n={n} ksel={ksel} p={p} fused"))
        ws = a.workspace()
        report(a.check(p, ws, 0, f"mem_attn32 n={n} ksel={ksel} p={p} workspace"))
        assert torch.isnan(ws[-4:]).all(), "written past the workspace"
        if ksel > 1:
            o, ml = a.partials(ws, ksel)
            assert torch.isfinite(o).all() and torch.isfinite(ml).all(), "a partial row the combine reads was not written"
        else:
            assert torch.isnan(ws).all(), "one picked frame: the fused launch, the workspace is not used"


@pytest.mark.parametrize("ksel", R.ATTN64_KSEL)
@pytest.mark.parametrize("n", R.ATTN64_N)
def test_mem_attn_64_query_kernel(lib, n, ksel):
    """1, 2, 3 and 5 key tiles per frame (every prologue path of the LDS-DMA ring), workgroups whose waves 1-3 hold no query, every
    frames_per_workgroup 0 .. 5 with every ksel 1 .. 5 (values above ksel included: one split), T = 3: the renumbering of the workgroups
    must reach every (clip, query block, split) exactly once -- every partial row the combine reads is finite, every flag pair written,
    and none raised: with these inputs nothing is to be redone, so the result is the 64-query kernel's own.  Both p_formats.  The
    mf.hi == NULL form is run at frames_per_workgroup = 0 only: it lives in the combine kernel, which every value shares."""
    L, lb = lib, lib.load()
    a = _Attn(L, ("table", 64, n, ksel))
    g = (n + 255) // 256
    for frames in R.ATTN64_FRAMES:
        nsp = lb.ppms_mem_attn_splits(a.T, ksel, n, frames)
        if frames >= 1:
            assert nsp == -(-ksel // frames), (ksel, frames, nsp)
        else:
            assert nsp in (ksel, -(-ksel // 2))
        for p in (1, 0):
            ws = a.workspace()
            label = f"mem_attn64 n={n} ksel={ksel} frames={frames} p={p}"
            if frames == 0:
                report(a.check(p, ws, frames, label))
            else:
                raw, X = a.run(p, ws, frames)
                report(R.attn_check(a.name, p, raw, X.to_f32(MFG0, 128), label))
            o, ml = a.partials(ws, nsp)
            assert torch.isfinite(o).all() and torch.isfinite(ml).all(), "a partial row the combine reads was not written"
            flags, behind = a.flags(ws, nsp)
            assert flags.numel() == a.T * nsp * g * 2 and (flags != NAN_BITS).all(), "the flag table is not fully written"
            assert (flags == 0).all(), "a tile was flagged: no score of these inputs is 2^16 above another (the CPU test asserts it)"
            assert (behind == NAN_BITS).all() and torch.isnan(ws[-4:]).all(), "written behind the flag pairs of this launch"


@pytest.mark.parametrize("p_format", P_FORMATS)
@pytest.mark.parametrize("kernel", [32, 64])
def test_mem_attn_sharded_form(lib, kernel, p_format):
    """T = 2 clips of this rank, sel rows that pick among the Tg = 6 frames of vt (up to frame 5): both kernels, fused and with a workspace"""
    a = _Attn(lib, ("sharded", kernel))
    assert a.v.shape[0] == 6 and a.T == 2 and int(a.sel.max()) == 5
    if kernel == 32:
        report(a.check(p_format, None, 0, f"mem_attn sharded 32 p={p_format} fused"))
    for frames in ((0,) if kernel == 32 else (0, 1, 2)):
        report(a.check(p_format, a.workspace(), frames, f"mem_attn sharded {kernel} p={p_format} workspace frames={frames}"))


@pytest.mark.parametrize("p_format", P_FORMATS)
@pytest.mark.parametrize("frames", R.FIXUP_FRAMES)
def test_mem_attn_fixup_of_one_tile(lib, frames, p_format):
    """the dominating-key construction at n = 320, T = 2, ksel = 5: the boosted keys sit in slot 2 and belong to the queries of the partly
    filled second 256-query block of clip 0 (the first block's queries meet them with a score of exactly 0).  The flag of exactly that
    (clip, split, block) is raised -- the split in the middle with one frame per workgroup, the first one's last frame with three -- and
    the fix-up pass leaves the result inside the same bound."""
    L, lb = lib, lib.load()
    a = _Attn(L, ("fixup",))
    nsp = lb.ppms_mem_attn_splits(a.T, a.ksel, a.n, frames)
    assert nsp == -(-a.ksel // frames)
    ws = a.workspace()
    raw, X = a.run(p_format, ws, frames)
    flags, _ = a.flags(ws, nsp)
    want = torch.zeros_like(flags)
    want[0, R.FIXUP_SLOT // frames, 1] = 1
    assert torch.equal(flags, want), flags.cpu().tolist()
    o, ml = a.partials(ws, nsp)
    assert torch.isfinite(o).all() and torch.isfinite(ml).all()
    report(R.attn_check(a.name, p_format, raw, X.to_f32(MFG0, 128), f"mem_attn fix-up frames={frames} p={p_format}"))


def test_mem_attn_refuses_misaligned_operands(lib):
    """qb, kb, out_bf16, the workspace and the planes of mf / mfg are accessed 16 bytes at a time, and so is vt where n % 8 == 0: a pointer
    that is not 16-byte aligned is refused with PPMS_EINVAL and the refusal's message; nothing is launched"""
    L, lb, s = lib, lib.load(), lib.stream_ptr()
    a = _Attn(L, ("table", 64, 64, 2))
    T, n, ksel = a.T, a.n, a.ksel
    X = sp_out(L, T * n, XC)
    raw, ws = bf16_out(T * n * 128), a.workspace()
    vt = a.vt_for(0)
    ok = dict(qb=a.qb.data_ptr(), kb=a.kb.data_ptr(), vt=vt.data_ptr(), mf=X.view(MF0, 128), mfg=X.view(MFG0, 128), raw=raw.data_ptr(), ws=ws.data_ptr())

    def call(**kw):
        v = dict(ok, **kw)
        return lb.ppms_mem_attn(v["qb"], v["kb"], v["vt"], a.sel.data_ptr(), ksel, a.scale, a.beta.data_ptr(), v["mf"], v["mfg"], v["raw"], T, n, v["ws"], 0, 0, s)

    for name in ("qb", "kb", "vt", "raw", "ws"):
        refused(L, call(**{name: ok[name] + 8}), "mem_attn: qb, kb, out_bf16, split_ws .*16-byte aligned")
    for name, c0 in (("mf", MF0 + 4), ("mfg", MFG0 + 4)):
        assert X.view(c0, 128).hi % 16 == 8
        refused(L, call(**{name: X.view(c0, 128)}), "16-B aligned SP views")
    torch.cuda.synchronize()
    assert planes_are(X, 0, XC, R.SENTINEL) and untouched(raw) and torch.isnan(ws).all(), "a refused call must not launch"
