"""Descriptor-driven float64 reference for the planned convolution launches (helper of tests/test_gpu_plan_audit.py,
tests/test_gpu_plan_audit_geometries.py and tests/test_conv_audit_ref.py; not a test module itself).

Given a ``ConvOp`` (or a bare ``ppms_conv`` descriptor with its kernel identity) and the objects that own its buffers, this module

* resolves every pointer the kernel will dereference to (storage, element offset) over the tensors reachable from the owners, and checks
  that every extent the kernel touches -- input rows with their temporal halo slabs, output rows x n_valid, V^T, the packed weights --
  lies inside its storage (a descriptor that fails is never launched);
* unpacks the weights from the pack the kernel reads, using only the kernel identity and the descriptor (never the state_dict);
* fills the input storages with seeded random finite data (every byte, neighbouring channels, padding and halo rows included) and the
  output-only storages with a NaN pattern;
* computes the reference in float64 (im2col gather + matmul, then the epilogue of include/ppms.h) on a pixel sample whose full rows and
  columns cross every tile boundary of any tiling;
* and checks a launch: accuracy on the sample, no byte changed outside the declared output regions, no read/write overlap, the split-bf16
  representation of SP outputs, bitwise determinism.

The last section audits whole engines: every planned launch of the engines of one geometry (``audit_geometry``), with a census of what the
planner chose for which conv (``Census``), which the geometry audit's conditions read.
"""
from __future__ import annotations

import bisect
import collections
import ctypes as C
import gc
import math
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from ppmstereo_amd import _lib as L
from ppmstereo_amd import packing as P
from ppmstereo_amd import convplan
from ppmstereo_amd.convplan import CONV2, CONV5, CONV6, GEMM1, KERNEL_NAMES, STREAM, ConvOp, kernel_record, sweep_taps
from ppmstereo_amd.dist import FrameShard

ACC_MAX = 3e-5      # per epilogue half: max |got - ref| <= ACC_MAX * max(1, max |ref|)  (the kernel tests' bound, tests/test_gpu_ops.py)
ACC_RMS = 2e-5      # and rms(got - ref) <= ACC_RMS * rms(ref)
FULL_SAMPLE = 65536  # volumes up to this many pixels are checked at every pixel


class AuditError(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------ pointer resolution
class Pool:
    """Every live tensor storage reachable from the owners (attributes walked recursively: tensors, SPTensor.data, lists, dicts, the
    package's own objects, ConvOp.keep) with a name path for messages.  ``resolve(ptr)`` -> (storage key, byte offset) or None."""

    def __init__(self, *owners, extra: Sequence[torch.Tensor] = ()):
        self.st: Dict[int, dict] = {}
        self.convops: List[ConvOp] = []
        seen = set()
        for i, o in enumerate(owners):
            self._walk(o, f"owner{i}", seen)
        for i, t in enumerate(extra):
            self._add(t, f"extra{i}")
        self._keys = sorted(self.st)

    def _add(self, t: torch.Tensor, name: str):
        s = t.untyped_storage()
        base, nb = s.data_ptr(), s.nbytes()
        if nb == 0 or base in self.st:
            return
        self.st[base] = dict(nbytes=nb, t=t, name=name, device=t.device)

    def _walk(self, o, name, seen):
        if o is None or isinstance(o, (int, float, str, bool, C._SimpleCData, C.Structure, C.Array)):
            return
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            self._add(o, name)
        elif isinstance(o, dict):
            for k, v in list(o.items()):
                self._walk(v, f"{name}[{k!r}]", seen)
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                self._walk(v, f"{name}[{i}]", seen)
        elif type(o).__module__.startswith(("ppmstereo_amd", "conv_audit", "test_")) and hasattr(o, "__dict__"):
            if isinstance(o, ConvOp):
                self.convops.append(o)
            for k, v in vars(o).items():
                self._walk(v, f"{name}.{k}", seen)

    def resolve(self, ptr: int):
        i = bisect.bisect_right(self._keys, ptr) - 1
        if i < 0:
            return None
        base = self._keys[i]
        if ptr >= base + self.st[base]["nbytes"]:
            return None
        return base, ptr - base

    def bytes(self, key: int) -> torch.Tensor:
        """The whole storage as a flat uint8 tensor."""
        e = self.st[key]
        if "flat" not in e:
            t = e["t"]
            n = e["nbytes"] // t.element_size()
            e["flat"] = t.as_strided((n,), (1,), 0).view(torch.uint8)
        return e["flat"]

    def typed(self, key: int, dtype) -> torch.Tensor:
        b = self.bytes(key)
        es = torch.empty((), dtype=dtype).element_size()
        return b[: b.numel() // es * es].view(dtype)


class Region:
    """rows x cols elements of `dtype` at `ld` starting `row0` rows from pointer `ptr` (row0 < 0: halo rows before it)."""

    def __init__(self, name, role, ptr, dtype, rows, ld, cols, row0=0, kind=None):
        self.name, self.role, self.ptr, self.dtype, self.rows, self.ld, self.cols, self.row0, self.kind = \
            name, role, ptr, dtype, rows, ld, cols, row0, kind
        self.es = torch.empty((), dtype=dtype).element_size()
        self.key = self.off = None          # storage key, element offset of the first touched element

    def bind(self, pool: Pool) -> Optional[str]:
        if not self.ptr:
            return f"{self.name}: NULL pointer"
        r = pool.resolve(self.ptr)
        if r is None:
            return f"{self.name}: pointer {self.ptr:#x} lies in no live tensor of the owners"
        key, boff = r
        if boff % self.es:
            return f"{self.name}: pointer misaligned for {self.dtype}"
        if self.rows > 1 and self.cols > self.ld:
            return f"{self.name}: {self.cols} columns exceed ld {self.ld}"
        n = pool.st[key]["nbytes"] // self.es
        off = boff // self.es + self.row0 * self.ld
        last = off + (self.rows - 1) * self.ld + self.cols
        if off < 0 or last > n:
            return (f"{self.name}: extent [{off}, {last}) elements of {self.dtype} outside {pool.st[key]['name']} "
                    f"({n} elements; {self.rows} rows x {self.cols} at ld {self.ld}, first row {self.row0})")
        self.key, self.off = key, off
        return None

    def view(self, pool: Pool) -> torch.Tensor:
        return pool.typed(self.key, self.dtype).as_strided((self.rows, self.cols), (self.ld, 1), self.off)

    def bytes_span(self):
        b0 = self.off * self.es
        return b0, self.ld * self.es, self.rows, self.cols * self.es

    def overlaps(self, o: "Region") -> bool:
        if self.key != o.key:
            return False
        a, sa, na, wa = self.bytes_span()
        b, sb, nb, wb = o.bytes_span()
        if na == 1:
            sa = max(sa, wa)
        if nb == 1:
            sb = max(sb, wb)
        if sa != sb or wa > sa or wb > sb:                      # different strides: the enclosing byte intervals
            return a < b + (nb - 1) * sb + wb and b < a + (na - 1) * sa + wa
        if b < a:
            a, b, na, nb, wa, wb = b, a, nb, na, wb, wa
        q, rem = divmod(b - a, sa)
        rows_meet = lambda r0: max(r0, 0) < min(r0 + nb, na)
        if rows_meet(q) and rem < wa:
            return True
        return rem + wb > sa and rows_meet(q + 1) and 0 < wa        # B's rows spill into A's next row


def _halves(d):
    return [0] + ([1] if d.m_split < d.M else [])


def _seg_k(d) -> int:
    return d.seg[0].c if d.groups == 2 else sum(d.seg[i].c for i in range(d.nseg))


def weight_elems(d) -> int:
    """bf16 elements of every pack layout: 2 planes x taps x padded K x M (packing.py)."""
    return 2 * d.kt * d.kh * d.kw * _seg_k(d) * d.M


def regions(d) -> List[Region]:
    """Every memory range the kernel of descriptor d reads or writes."""
    T, HW = d.T, d.H * d.W
    Pn = T * HW
    th = d.t_halo
    bf, f32 = torch.bfloat16, torch.float32
    out: List[Region] = []
    for i in range(d.nseg):
        s = d.seg[i]
        for pl in ("hi", "lo"):
            out.append(Region(f"seg[{i}].{pl}", "in", getattr(s, pl), bf, (T + 2 * th) * HW, s.ld, s.c, -th * HW, kind="sp"))
    out.append(Region("w", "w", d.w, bf, 1, weight_elems(d), weight_elems(d)))
    out.append(Region("bias", "w", d.bias, f32, 1, d.M, d.M))
    for h in _halves(d):
        e = d.epi[h]
        nv = e.n_valid
        p = f"epi[{h}]."
        if e.kind != L.EPI_ADDF32 and e.out_sp.hi:
            for pl in ("hi", "lo"):
                out.append(Region(p + "out_sp." + pl, "out", getattr(e.out_sp, pl), bf, Pn, e.out_sp.ld, nv, kind="sp"))
        if e.out_f32:
            out.append(Region(p + "out_f32", "inout" if e.kind == L.EPI_ADDF32 else "out", e.out_f32, f32, Pn, e.out_f32_ld, nv))
        if e.kind == L.EPI_STORE and e.out_vt:
            out.append(Region(p + "out_vt", "out", e.out_vt, bf, 1, T * nv * HW, T * nv * HW))
        if e.kind in (L.EPI_RESID, L.EPI_RH, L.EPI_GRU):
            for pl in ("hi", "lo"):
                out.append(Region(p + "aux_sp." + pl, "in", getattr(e.aux_sp, pl), bf, Pn, e.aux_sp.ld, nv, kind="sp"))
        if e.kind == L.EPI_GRU:
            out.append(Region(p + "aux_f32", "in", e.aux_f32, f32, Pn, e.aux_f32_ld, nv, kind="z"))
        if e.pre_f32:
            out.append(Region(p + "pre_f32", "in", e.pre_f32, f32, Pn, e.pre_f32_ld, nv))
    return out


def bind_regions(d, pool: Pool, allowed_overlaps=()) -> (List[Region], List[str]):
    """(regions, problems): unresolved pointers, extents outside their storage, halves that do not fit, read/write overlaps."""
    errs = []
    if d.m_split < d.M:
        if d.epi[0].n_valid > d.m_split or d.epi[1].n_valid > d.M - d.m_split:
            errs.append(f"n_valid ({d.epi[0].n_valid}, {d.epi[1].n_valid}) does not fit the halves of M = {d.M} split at {d.m_split}")
    elif d.epi[0].n_valid > d.M:
        errs.append(f"n_valid {d.epi[0].n_valid} > M = {d.M}")
    rs = regions(d)
    for r in rs:
        msg = r.bind(pool)
        if msg:
            errs.append(msg)
    if not errs:
        outs = [r for r in rs if r.role in ("out", "inout")]
        ins = [r for r in rs if r.role in ("in", "w")]
        for o in outs:
            for i in ins:
                if o.overlaps(i) and (o.name, i.name) not in allowed_overlaps:
                    errs.append(f"output {o.name} overlaps input {i.name} in {pool.st[o.key]['name']}")
        for a in range(len(outs)):
            for b in range(a + 1, len(outs)):
                if outs[a].overlaps(outs[b]):
                    errs.append(f"outputs {outs[a].name} and {outs[b].name} overlap")
    return rs, errs


# ------------------------------------------------------------------------------------------------ weights from the pack
def swept(version: int, ysweep: bool, d) -> bool:
    return kernel_record(version, ysweep).swept and (d.kh > 1 or d.kw > 1)


# the hand-written inverse of every layout (packing.py) as (packed, M, tap shape of the pack, chunks of the kernel's granule) -> fp32 [M][K]
UNPACK = {
    CONV2: lambda p, M, pt, n: P.unpack_conv2_reference(p, M, math.prod(pt) * n, pt, n),
    CONV5: lambda p, M, pt, n: P.unpack_conv5_reference(p, M, math.prod(pt) * n, pt, n),
    CONV6: lambda p, M, pt, n: P.unpack_conv6_reference(p, M, math.prod(pt) * n, pt, n),
    GEMM1: lambda p, M, pt, n: P.unpack_gemm1_reference(p, M, n),
    STREAM: lambda p, M, pt, n: P.unpack_stream_reference(p, M, math.prod(pt), n),
}


def unpack_weights(version: int, ysweep: bool, d, packed: torch.Tensor, sweep_inverse: bool = True) -> torch.Tensor:
    """float64 (M, K, kt, kh, kw) weights the kernel multiplies (hi + lo of the pack), K = the padded input channels of the launch (one
    group's for groups == 2: rows [0, m_split) read seg[0], the rest seg[1]).  sweep_inverse False: read a sweep-ordered pack as if it
    were in natural tap order (a deliberately wrong reference, for the self-checks)."""
    kt, kh, kw = d.kt, d.kh, d.kw
    K, M = _seg_k(d), d.M
    taps = kt * kh * kw
    packed = packed.reshape(-1)
    assert packed.numel() == weight_elems(d)
    if version not in UNPACK:
        raise AuditError(f"unknown kernel version {version}")
    sw = swept(version, ysweep, d) and sweep_inverse
    pt = sweep_taps(kt, kh, kw) if sw else (kt, kh, kw)
    assert version != GEMM1 or taps == 1
    wm = UNPACK[version](packed, M, pt, K // kernel_record(version, ysweep).granule)
    w = wm.double().reshape(M, *pt, K).permute(0, 4, 1, 2, 3)          # (M, K, kt, pt1, pt2): the pack's own (sweep) order
    if sw:
        w = convplan.sweep_inverse(w, (kt, kh, kw))
    return w.contiguous()


# ------------------------------------------------------------------------------------------------ inputs
def _gen(n: int, g: torch.Generator, device, kind: str) -> torch.Tensor:
    if kind == "z":
        return torch.rand(n, generator=g, device=device) * 0.98 + 0.01
    return torch.randn(n, generator=g, device=device)


def fill_storages(pool: Pool, rs: List[Region], d, seed: int):
    """Inputs: every byte of every storage an input pointer resolves into gets seeded random finite data (SP storages as consistent
    hi / lo pairs, lo == 0 from lo_zero_from on; z in (0, 1); pre_f32 / aux random).  Output-only storages: all-ones bf16 / fp32 NaN
    bit patterns, so that an element the kernel does not write shows up."""
    ins = {}
    for r in rs:
        if r.role in ("in", "inout"):
            ins.setdefault(r.key, []).append(r)
    dev = next(iter(pool.st.values()))["device"]
    g = torch.Generator(device=dev)
    for key, lst in sorted(ins.items()):
        g.manual_seed(seed * 7919 + (key % 104729))
        kinds = {r.kind for r in lst}
        if "sp" in kinds:
            hi = next(r for r in lst if r.kind == "sp" and r.name.endswith(".hi"))
            lo = next(r for r in lst if r.kind == "sp" and r.name.endswith(".lo") and r.name[:-3] == hi.name[:-3])
            flat = pool.typed(key, torch.bfloat16)
            plane = (lo.ptr - hi.ptr) // 2
            assert plane > 0 and 2 * plane == flat.numel(), f"{pool.st[key]['name']}: not a two-plane SP storage"
            CH = 1 << 26
            for a in range(0, plane, CH):
                n = min(CH, plane - a)
                x = _gen(n, g, dev, "sp")
                h = x.to(torch.bfloat16)
                flat[a:a + n] = h
                flat[plane + a:plane + a + n] = (x - h.float()).to(torch.bfloat16)
            if d.lo_zero_from > 0:
                cs = 0
                for i in range(d.nseg):
                    s = d.seg[i]
                    a0 = max(d.lo_zero_from - cs, 0)
                    if a0 < s.c and pool.resolve(s.hi)[0] == key:
                        c0 = (pool.resolve(s.hi)[1] // 2) % s.ld
                        flat[plane:].view(-1, s.ld)[:, c0 + a0:c0 + s.c] = 0
                    cs += s.c
        else:
            flat = pool.typed(key, torch.float32)
            CH = 1 << 26
            kind = "z" if "z" in kinds else "f"
            for a in range(0, flat.numel(), CH):
                n = min(CH, flat.numel() - a)
                flat[a:a + n] = _gen(n, g, dev, kind)
    for r in rs:
        if r.role == "out" and r.key not in ins:
            pool.bytes(r.key).fill_(0xFF)


# ------------------------------------------------------------------------------------------------ sample + reference
def pixel_sample(T: int, H: int, W: int, seed: int, device) -> torch.Tensor:
    n = T * H * W
    if n <= FULL_SAMPLE:
        return torch.arange(n, device=device)
    HW = H * W
    idx = []
    frames = sorted({0, 1, T // 2, T - 2, T - 1} & set(range(T)))
    rows = sorted({0, 1, 2, H // 2, H - 3, H - 2, H - 1} & set(range(H)))
    cols = sorted({0, 1, W // 2, W - 2, W - 1} & set(range(W)))
    xs, ys = torch.arange(W), torch.arange(H)
    for t in frames:
        for y in rows:
            idx.append(t * HW + y * W + xs)
        for x in cols:
            idx.append(t * HW + ys * W + x)
    g = torch.Generator().manual_seed(seed)
    for _ in range(8):
        t, y = int(torch.randint(T, (1,), generator=g)), int(torch.randint(H, (1,), generator=g))
        idx.append(t * HW + y * W + xs)
    idx.append(torch.arange(n - min(4096, n), n))
    return torch.unique(torch.cat(idx)).to(device)


def _act(v: torch.Tensor, act: int) -> torch.Tensor:
    if act == L.ACT_NONE:
        return v
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == L.ACT_TANH:
        return torch.tanh(v)
    if act == L.ACT_ELU1:
        return torch.where(v > 0, v + 1.0, torch.exp(v))
    raise AuditError(f"unknown activation {act}")


def _gather_rows(view_hi, view_lo, rows: torch.Tensor) -> torch.Tensor:
    return view_hi[rows].double() + view_lo[rows].double()


def reference(d, version: int, ysweep: bool, pool: Pool, rs: List[Region], pix: torch.Tensor, sweep_inverse: bool = True,
              halo_zero: bool = False, wcache: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """float64 expected values at the sample pixels, per output region name: 'epi[h].out_sp' / 'epi[h].out_f32' -> (n, n_valid);
    'epi[h].out_vt' -> (n, n_valid) (values before the 16-bit encoding).  halo_zero: treat the halo slabs as zero padding (a deliberately
    wrong reference, for the self-checks)."""
    byname = {r.name: r for r in rs}
    T, H, W, HW = d.T, d.H, d.W, d.H * d.W
    th = 0 if halo_zero else d.t_halo
    dev = pix.device
    key = (d.w, version, ysweep, d.kt, d.kh, d.kw, d.M, _seg_k(d), sweep_inverse)
    if wcache is not None and key in wcache:
        w5 = wcache[key]
    else:
        w5 = unpack_weights(version, ysweep, d, byname["w"].view(pool)[0], sweep_inverse).to(dev)
        if wcache is not None:
            wcache[key] = w5
    bias = byname["bias"].view(pool)[0].double()
    M, taps = d.M, d.kt * d.kh * d.kw
    t, rem = pix // HW, pix % HW
    y, x = rem // W, rem % W
    segv = []
    for i in range(d.nseg):
        segv.append((byname[f"seg[{i}].hi"].view(pool), byname[f"seg[{i}].lo"].view(pool)))   # rows from -t_halo * HW
    K = _seg_k(d)
    wmat = w5.permute(0, 2, 3, 4, 1).reshape(M, taps * K)                 # [m][tap * K + ci]
    n = pix.numel()
    chunk = max(256, (1 << 25) // (taps * sum(d.seg[i].c for i in range(d.nseg))))
    acc = torch.empty(n, M, dtype=torch.float64, device=dev)
    dz, dy, dx = torch.meshgrid(torch.arange(d.kt, device=dev) - d.kt // 2, torch.arange(d.kh, device=dev) - d.kh // 2,
                                torch.arange(d.kw, device=dev) - d.kw // 2, indexing="ij")
    dz, dy, dx = dz.reshape(-1), dy.reshape(-1), dx.reshape(-1)
    for a in range(0, n, chunk):
        sl = slice(a, min(n, a + chunk))
        ts, ys_, xs_ = t[sl, None] + dz, y[sl, None] + dy, x[sl, None] + dx           # (n, taps)
        ok = (ys_ >= 0) & (ys_ < H) & (xs_ >= 0) & (xs_ < W) & (ts >= -th) & (ts < T + th)
        rows = torch.where(ok, (ts + d.t_halo) * HW + ys_ * W + xs_, torch.zeros_like(ts)).reshape(-1)
        parts = []
        for vh, vl in segv:
            g_ = _gather_rows(vh, vl, rows).reshape(ok.shape[0], taps, -1) * ok[..., None]
            parts.append(g_)
        if d.groups == 2:
            ms = d.m_split
            acc[sl, :ms] = parts[0].reshape(-1, taps * K) @ wmat[:ms].T
            acc[sl, ms:] = parts[1].reshape(-1, taps * K) @ wmat[ms:].T
        else:
            acc[sl] = torch.cat(parts, 2).reshape(-1, taps * K) @ wmat.T
    acc += bias
    exp = {}
    for h in _halves(d):
        e = d.epi[h]
        m0 = 0 if h == 0 else d.m_split
        nv = e.n_valid
        p = f"epi[{h}]."
        v = acc[:, m0:m0 + nv]
        if e.pre_f32:
            v = v + byname[p + "pre_f32"].view(pool)[pix].double()
        if e.kind == L.EPI_STORE:
            yv = _act(v, e.act) * e.scale
        elif e.kind == L.EPI_RESID:
            aux = _gather_rows(byname[p + "aux_sp.hi"].view(pool), byname[p + "aux_sp.lo"].view(pool), pix)
            yv = _act(aux + v, e.act) * e.scale
        elif e.kind == L.EPI_RH:
            aux = _gather_rows(byname[p + "aux_sp.hi"].view(pool), byname[p + "aux_sp.lo"].view(pool), pix)
            yv = torch.sigmoid(v) * aux
        elif e.kind == L.EPI_GRU:
            aux = _gather_rows(byname[p + "aux_sp.hi"].view(pool), byname[p + "aux_sp.lo"].view(pool), pix)
            z = byname[p + "aux_f32"].view(pool)[pix].double()
            yv = (1.0 - z) * aux + z * torch.tanh(v)
        elif e.kind == L.EPI_ADDF32:
            yv = byname[p + "out_f32"].view(pool)[pix].double() + v
        else:
            raise AuditError(f"unknown epilogue kind {e.kind}")
        for r in (p + "out_sp.hi", p + "out_f32", p + "out_vt"):
            if r in byname:
                exp[r.replace(".hi", "")] = yv
    return exp


def got_values(d, pool: Pool, rs: List[Region], pix: torch.Tensor) -> Dict[str, torch.Tensor]:
    byname = {r.name: r for r in rs}
    HW = d.H * d.W
    got = {}
    for h in _halves(d):
        p = f"epi[{h}]."
        nv = d.epi[h].n_valid
        if p + "out_sp.hi" in byname:
            got[p + "out_sp"] = _gather_rows(byname[p + "out_sp.hi"].view(pool), byname[p + "out_sp.lo"].view(pool), pix)
        if p + "out_f32" in byname:
            got[p + "out_f32"] = byname[p + "out_f32"].view(pool)[pix].double()
        if p + "out_vt" in byname:
            vt = byname[p + "out_vt"].view(pool).reshape(d.T, nv, HW)
            got[p + "out_vt"] = L.vt_values(vt[pix // HW, :, pix % HW], d.epi[h].vt_f16).double()
    return got


def compare(exp: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor], d, ratios: Optional[dict] = None) -> (List[str], Dict[str, List[int]]):
    """(failures, bad couts per output) under the per-half bounds.  ratios (optional dict): receives output name -> the measured max error / its bound."""
    fails, bad = [], {}
    for name, ref in exp.items():
        g = got[name]
        err = (g - ref).abs()
        amax = ref.abs().max().item() if ref.numel() else 0.0
        tol = ACC_MAX * max(1.0, amax)
        if name.endswith("out_vt"):        # bf16(y) (or its fp16 image): half an ulp of bf16 on top (fp16 subnormals: 2^-25 absolute)
            err = err - (ref.abs() * 2.0 ** -8 + 2.0 ** -24)
        colmax = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err).amax(0) if err.numel() else err
        cols = torch.nonzero(~(colmax <= tol)).reshape(-1).tolist()
        if ratios is not None and err.numel():
            ratios[name] = colmax.max().item() / tol
        if cols:
            bad[name] = cols
            fails.append(f"{name}: max err {colmax.max().item():.3e} > {tol:.3e} at couts {cols[:16]}{' ...' if len(cols) > 16 else ''}")
        if not name.endswith("out_vt") and ref.numel():
            rms_e = err.pow(2).mean().sqrt().item()
            rms_r = ref.pow(2).mean().sqrt().item()
            if not rms_e <= ACC_RMS * rms_r:
                fails.append(f"{name}: rms err {rms_e:.3e} > {ACC_RMS} * rms(ref) {rms_r:.3e}")
    return fails, bad


# ------------------------------------------------------------------------------------------------ one launch
def kernel_name(op: ConvOp) -> str:
    return KERNEL_NAMES[op.version]


class Report:
    def __init__(self, name, op):
        d = op.desc
        self.name, self.kernel = name, kernel_name(op)
        self.conv = name.rsplit(":", 1)[-1]          # the conv's own name ("engine tag:conv")
        self.sliced = op.nslice > 1
        self.swept = swept(op.version, op.ysweep, d)
        self.halo = d.t_halo > 0
        # what the planner decided, and the facts of the descriptor its thresholds look at (the census conditions of the geometry audit)
        self.nslice, self.ysweep = int(op.nslice), bool(op.ysweep)
        self.pixels = d.T * d.H * d.W
        self.taps = (d.kt, d.kh, d.kw)
        self.couts = d.epi[0].n_valid + (d.epi[1].n_valid if d.m_split < d.M else 0)
        self.vt = any(d.epi[h].kind == L.EPI_STORE and bool(d.epi[h].out_vt) for h in _halves(d))
        self.worst = 0.0                             # worst max-error / bound over the outputs of the launch (compare())
        self.launched = False
        self.failures: List[str] = []
        self.bad: Dict[str, List[int]] = {}

    def __str__(self):
        return f"{self.name} [{self.kernel}{' sliced' if self.sliced else ''}{' swept' if self.swept else ''}{' halo' if self.halo else ''}]: " + \
            ("; ".join(self.failures) if self.failures else "ok")


def audit_op(name: str, op: ConvOp, pool: Pool, seed: int = 0, ref_desc=None, wcache: Optional[dict] = None,
             allowed_overlaps=()) -> Report:
    """Audit one launch of `op`.  The reference is computed from `ref_desc` (default: op.desc) -- the sensitivity test launches a
    perturbed descriptor against the reference of the original one."""
    rep = Report(name, op)
    d = op.desc
    rd = d if ref_desc is None else ref_desc
    rs, errs = bind_regions(d, pool, allowed_overlaps)
    if ref_desc is not None:
        rrs, rerrs = bind_regions(rd, pool, allowed_overlaps)
        errs += rerrs
    else:
        rrs = rs
    if errs:                                          # never launch a descriptor whose extents were not all verified
        rep.failures += errs
        return rep
    fill_storages(pool, rs, d, seed)
    keys = sorted({r.key for r in rs} | {r.key for r in rrs})
    snap = {k: pool.bytes(k).clone() for k in keys}
    pix = pixel_sample(d.T, d.H, d.W, seed, pix_device(pool))
    exp = reference(rd, op.version, op.ysweep, pool, rrs, pix, wcache=wcache)
    op()
    torch.cuda.synchronize()
    rep.launched = True
    # 1. accuracy on the sample
    ratios = {}
    f, bad = compare(exp, got_values(d, pool, rs, pix), d, ratios)
    rep.failures += f
    rep.bad = bad
    rep.worst = max(ratios.values(), default=0.0)
    # 2. no byte changed outside the declared output regions (inputs, halo rows, padded couts, neighbouring channels)
    outs = [r for r in rs if r.role in ("out", "inout")]
    for r in outs:
        full = r.view(pool)
        if not torch.isfinite(full.float()).all():
            bad_rows = torch.nonzero(~torch.isfinite(full.float()).all(1)).reshape(-1)
            rep.failures.append(f"{r.name}: {bad_rows.numel()} rows with non-finite values (not written?), first pixel {bad_rows[0].item()}")
        snap_t = snap[r.key][: snap[r.key].numel() // r.es * r.es].view(r.dtype).as_strided((r.rows, r.cols), (r.ld, 1), r.off)
        snap_t.copy_(full)
    for k in keys:
        now = pool.bytes(k)
        first = _first_difference(now, snap[k])
        if first is not None:
            rep.failures.append(f"bytes of {pool.st[k]['name']} changed outside the declared outputs (first at byte {first} of {now.numel()})")
    # 4. the SP representation: hi == RNE-bf16(hi + lo); out_sp and out_f32 agree where both are set
    byname = {r.name: r for r in rs}
    for h in _halves(d):
        p = f"epi[{h}]."
        if p + "out_sp.hi" in byname:
            hi, lo = byname[p + "out_sp.hi"].view(pool), byname[p + "out_sp.lo"].view(pool)
            f32 = byname[p + "out_f32"].view(pool) if p + "out_f32" in byname else None
            bad = disagree = 0
            for a in range(0, hi.shape[0], CHUNK_ROWS):
                h_, l_ = hi[a:a + CHUNK_ROWS], lo[a:a + CHUNK_ROWS]
                bad += sp_split_violations(h_, l_)
                if f32 is not None:
                    f_ = f32[a:a + CHUNK_ROWS]
                    disagree += int((~((h_.float() + l_.float() - f_).abs() <= f_.abs() * 2.0 ** -15 + 1e-30)).sum().item())
            if bad:
                rep.failures.append(f"{p}out_sp: {bad} elements with hi != bf16(hi + lo)")
            if disagree:
                rep.failures.append(f"{p}out_sp and {p}out_f32 disagree at {disagree} elements")
    # 5. determinism: the same inputs give the same bits
    if not any(r.role == "inout" for r in rs):
        first = {r.key: pool.bytes(r.key).clone() for r in outs}
        op()
        torch.cuda.synchronize()
        for k, v in first.items():
            if _first_difference(pool.bytes(k), v) is not None:
                rep.failures.append(f"second launch changed {pool.st[k]['name']}: not deterministic")
    return rep


CHUNK_ROWS = 1 << 20


def _first_difference(a: torch.Tensor, b: torch.Tensor, chunk: int = 1 << 28) -> Optional[int]:
    """Index of the first differing byte of two flat uint8 tensors (None: equal), compared in chunks (bounded temporaries)."""
    for i in range(0, a.numel(), chunk):
        x, y = a[i:i + chunk], b[i:i + chunk]
        if not torch.equal(x, y):
            return i + int(torch.nonzero(x != y)[0, 0].item())
    return None


def sp_split_violations(hi: torch.Tensor, lo: torch.Tensor) -> int:
    """Elements of a split-bf16 pair that are not hi = RNE-bf16(x), lo = RNE-bf16(x - hi) of some x: hi must be RNE-bf16(hi + lo) --
    except where lo is exactly half an ulp of hi (lo's own rounding can land there), which makes hi + lo a tie that RNE sends to the even
    neighbour; there hi must be the other neighbour, exactly 2 |lo| away."""
    r = (hi.float() + lo.float()).to(torch.bfloat16)
    same = r.view(torch.int16) == hi.view(torch.int16)
    tie = (hi.float() - r.float()).abs() == 2.0 * lo.float().abs()
    return int((~(same | tie)).sum().item())


def pix_device(pool: Pool):
    return next(iter(pool.st.values()))["device"]


def conv_ops(obj) -> Dict[str, ConvOp]:
    """name -> ConvOp of an engine: ScaleEngine.conv_family_ops() (ConvOps only), or the ops / steps lists of fnet / cnet / SST."""
    if hasattr(obj, "conv_family_ops"):
        return {k: v for k, v in obj.conv_family_ops().items() if isinstance(v, ConvOp)}
    seq = getattr(obj, "ops", None)
    if seq is not None:
        seq = [v for _, v in seq]
    else:
        seq = obj.steps
    return {f"{type(obj).__name__}[{i}]": v for i, v in enumerate(seq) if isinstance(v, ConvOp)}


# ------------------------------------------------------------------------------------------------ whole engines (the plan audits)
class HaloGeometry:
    """What a ScaleEngine reads from a dist.FrameShard to lay out a rank's window (f of f * world frames, halo slabs of FrameShard.HALO frames
    on both sides) -- and nothing else: the audit never exchanges data, so any other attribute access is an error."""

    HALO = FrameShard.HALO

    def __init__(self, f=5, world=8, rank=3):
        self.rank, self.world, self.f, self.T = rank, world, f, f * world
        self.lo, self.hi = rank * f, (rank + 1) * f
        self.group, self.force_comm = None, False

    def __getattr__(self, name):
        raise AssertionError(f"the plan audit must not exchange data (FrameShard.{name})")


def release():
    """Free released engines now: a ScaleEngine sits in reference cycles (bound methods and closures in its launch table), so dropping the
    last reference frees its gigabytes only when the cyclic collector runs."""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()


class Launch(NamedTuple):
    """One audited launch as the census keeps it: what the planner chose for which conv, and the descriptor facts its thresholds read."""
    conv: str           # the conv's name in its engine ("zr1_0_x", "final_0", "_FnetEngine[3]")
    scale: int          # map divisor of the update block (4, 8, 16); 0: an encoder engine
    convex3d: bool
    kernel: str
    nslice: int
    ysweep: bool
    pixels: int         # P = T * H * W of the launch
    taps: tuple         # (kt, kh, kw)
    couts: int          # stored couts (both halves)
    vt: bool            # writes V^T
    halo: bool          # t_halo > 0
    worst: float        # max error / bound


class Census:
    def __init__(self):
        self.k = collections.OrderedDict()
        self.launches: List[Launch] = []

    def add(self, rep: Report, scale: int = 0, convex3d: bool = False):
        c = self.k.setdefault(rep.kernel, collections.Counter())
        c["n"] += 1
        c["sliced"] += rep.sliced
        c["swept"] += rep.swept
        c["halo"] += rep.halo
        self.launches.append(Launch(rep.conv, scale, convex3d, rep.kernel, rep.nslice, rep.ysweep, rep.pixels, rep.taps, rep.couts, rep.vt,
                                    rep.halo, rep.worst))

    def line(self):
        total = sum(c["n"] for c in self.k.values())
        return f"{total} launches: " + ", ".join(f"{k} {c['n']} (sliced {c['sliced']}, swept {c['swept']}, halo'd {c['halo']})" for k, c in sorted(self.k.items()))

    def served(self, kernel: str, scale: int) -> List[str]:
        """The convs `kernel` serves at an update block's scale, in launch order, each name once."""
        return list(dict.fromkeys(l.conv for l in self.launches if l.kernel == kernel and l.scale == scale))

    def plans(self) -> str:
        """What the thresholds decided: per kernel the K-slice plans in use (y: the y-swept form), the launches on either side of the 4096-pixel
        threshold of conv_stream / gemm1, and the worst measured max-error / bound."""
        by = collections.OrderedDict()
        for l in sorted(self.launches, key=lambda l: l.kernel):
            e = by.setdefault(l.kernel, dict(s=collections.Counter(), small=0, n=0, worst=0.0))
            e["s"][f"{'y' if l.ysweep else ''}s{l.nslice}"] += 1
            e["small"] += l.pixels <= 4096
            e["n"] += 1
            e["worst"] = max(e["worst"], l.worst)
        out = []
        for k, e in by.items():
            s = " ".join(f"{p} x{n}" for p, n in sorted(e["s"].items()))
            small = f", P <= 4096: {e['small']} of {e['n']}" if k in ("conv_stream", "gemm1") else ""
            out.append(f"{k} [{s}{small}; worst err/bound {e['worst']:.3f}]")
        return "; ".join(out)


def audit_engine(tag: str, eng, census: Census, fails: list, seed: int, scale: int = 0, convex3d: bool = False) -> int:
    ops = conv_ops(eng)
    pool = Pool(eng)
    present = {id(o) for o in pool.convops}
    assert len(present) == len(ops) and present == {id(o) for o in ops.values()}, \
        f"{tag}: {len(present)} ConvOps in the engine, {len(ops)} listed for the audit"
    wcache = {}
    for i, (name, op) in enumerate(ops.items()):
        rep = audit_op(f"{tag}:{name}", op, pool, seed=seed + i, wcache=wcache)
        census.add(rep, scale, convex3d)
        if rep.failures:
            fails.append(str(rep))
    return len(ops)


def audit_with_bias_entry_off(name: str, op: ConvOp, eng, k: int, out: str, seed: int) -> Report:
    """The audit's sensitivity on one launch of an engine: `op` must pass as it is; then the same descriptor is launched with a test-owned
    bias copy whose entry k (a row of the pack) is off by 2^-10 max |ref of output `out`| -- an in-bounds descriptor -- and audited against
    the reference of the ORIGINAL bias.  -> the report of that second audit (the caller asserts that it fails and names the cout)."""
    pool = Pool(eng)
    dev = pix_device(pool)
    rep = audit_op(name, op, pool, seed=seed)
    assert rep.launched and not rep.failures, str(rep)
    rs, errs = bind_regions(op.desc, pool)
    assert not errs
    fill_storages(pool, rs, op.desc, seed)
    pix = pixel_sample(op.desc.T, op.desc.H, op.desc.W, seed, dev)
    amax = reference(op.desc, op.version, op.ysweep, pool, rs, pix)[out].abs().max().item()
    bias = next(r for r in rs if r.name == "bias").view(pool)[0].clone()
    bias[k] += 2.0 ** -10 * amax
    d2 = L.Conv.from_buffer_copy(bytes(op.desc))
    d2.bias = bias.data_ptr()
    op2 = ConvOp(d2, op.keep + [bias], op.version, op.wm_hint, nslice=op.nslice, ysweep=op.ysweep, device=dev)
    assert (op2.version, op2.nslice, op2.ysweep) == (op.version, op.nslice, op.ysweep)
    return audit_op(f"{name} (bias entry {k} perturbed)", op2, Pool(eng, extra=[bias]), seed=seed, ref_desc=op.desc)


SCALES = (("update_block16", 16, 0), ("update_block08", 8, 1), ("update_block04", 4, 2))     # block, map divisor, Attention_qk index


def load_models(device) -> dict:
    """The hot path for both use_convex_3d values and the three encoder modules, with the synthetic weights, on `device`."""
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.cnet import Feature
    from ppmstereo_amd.encoder import BasicEncoder
    from ppmstereo_amd.ppmstereo import PPMStereoHotPath
    from ppmstereo_amd.sst import SSTBlock
    hot = {c3: PPMStereoHotPath(use_convex_3d=c3).load_hot_path_weights(Wm.hot_path_weights(use_convex_3d=c3)).to(device).eval() for c3 in (False, True)}
    fnet = BasicEncoder(output_dim=256, norm_fn="instance")
    fnet.load_state_dict(Wm.fnet_weights(), strict=True)
    cnet = Feature("tiny", 256)
    cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sst = SSTBlock()
    sst.load_state_dict(Wm.sst_weights(), strict=True)
    return dict(hot=hot, fnet=fnet.to(device).eval(), cnet=cnet.to(device).eval(), sst=sst.to(device).eval())


def audit_geometry(models: dict, name: str, T: int, H: int, W: int, convex=(False, True), encoders: bool = False, shard=None, device="cuda:0"):
    """Every planned conv launch of one geometry: the three ScaleEngines of each use_convex_3d value with their q/k projection, and (encoders)
    the fnet / cnet / SST engines.  T: frames this engine holds; shard: (world, rank) of a frame-sharded window whose rank holds T frames
    between halo slabs.  -> (census, failure lines, launches audited)."""
    from ppmstereo_amd.cnet import _CnetEngine
    from ppmstereo_amd.encoder import _FnetEngine
    from ppmstereo_amd.sst import _SstEngine
    release()                      # (also whatever engines earlier test files left to the cyclic collector)
    census, fails, audited = Census(), [], 0
    dev = torch.device(device)
    for c3 in convex:
        hot = models["hot"][c3]
        for blk_name, s, ai in SCALES:
            blk = getattr(hot, blk_name)
            geo = HaloGeometry(f=T, world=shard[0], rank=shard[1]) if shard is not None else None
            eng = blk.engine(T, H // s, W // s, dev, shard=geo)
            assert eng.halo == (FrameShard.HALO if shard is not None else 0)
            eng.qk_op(hot.att[ai].packed(dev))                   # the q/k projection begin() launches
            audited += audit_engine(f"{name}/{blk_name}{'/convex3d' if c3 else ''}", eng, census, fails, seed=1000 * s + 7 * c3, scale=s, convex3d=c3)
            del eng
            blk._engines.clear()
            release()
    if encoders:
        fnet, cnet, sst = models["fnet"], models["cnet"], models["sst"]
        eng = _FnetEngine(fnet._pack(dev), 2 * T, H, W, dev, 256)          # left + right images in one call (ppmstereo.py:618)
        audited += audit_engine(f"{name}/fnet", eng, census, fails, seed=11)
        del eng
        release()
        eng = _CnetEngine(cnet._pack(dev), T, H, W, dev)
        audited += audit_engine(f"{name}/cnet", eng, census, fails, seed=12)
        del eng
        release()
        eng = _SstEngine(sst._pack(dev), sst.time_embed.detach().float()[0], T, H // 16, W // 16, dev)
        audited += audit_engine(f"{name}/sst", eng, census, fails, seed=13)
        del eng
        release()
    assert audited == len(census.launches) == sum(c["n"] for c in census.k.values())
    return census, fails, audited
