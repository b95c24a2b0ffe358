"""Which HIP kernel runs a convolution, and the weight packs it reads: the one place where every engine (the update block's ScaleEngine,
fnet, cnet, the SST block) packs its conv weights and plans its launches.

A convolution is packed once (``pack_conv``: one pack per kernel the caller allows and the weight's shape suits) and planned once per
geometry (``plan_conv``: the first kernel, in a fixed order, whose pack exists and which the library rates for the descriptor).  The
result is a ``ConvOp``: the host descriptor, its device copy and the resolved entry point, launched on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, NamedTuple, Optional, Sequence

import torch

from . import _lib as L
from . import packing as _packing
# Kernel identities (ConvOp.version; bench.py and the tests read the plain ints).  KERNELS below holds the record of each.
from .packing import CONV2, CONV5, CONV6, GEMM1, STREAM

CONV2_SWEPT = "2s"  # (pack key only) conv_gemm2's one-window form: the swept weight order of a (kt, kh, 1) conv, launched as CONV2 with ysweep

# The measured-best settings that are still switches.  The product reads no environment variable.
TUNING = dict(
    conv6_grouped=True,   # the two 128 -> 128 (1,1,5) tails of convz1 / convr1 as ONE grouped conv_gemm6 launch (ppms_conv.groups = 2, M = 256 wave layout) where
                          # conv_gemm6 serves the map, instead of two M = 128 launches on two streams
    attn_p="fp16",        # format of the unnormalised probabilities P~ in the memory read-out's P~ V product (and of the V^T image the to_v conv writes):
                          # "fp16" = 11 significand bits, "bf16" = 8 (what flash-attention itself uses) at the same MFMA count.  The reference fixtures were
                          # generated with fp32 P (tools/gen_golden.py:89-95); with bf16 P~ the iters = 20 cascade ends 1.3e-3 px from them, with fp16 inside 1e-3
)

# Per-launch HIP events (ConvOp.events, Engine.enable_attn_timing) are only recorded while this is on: bench.py samples them in a
# subset of its timed steps -- every event pair is two more packets in the queue, and with ~330 of them per clip the clip gets ~5 % slower.
KERNEL_TIMING = {"on": True}


def attn_p_format() -> int:
    """TUNING["attn_p"] as ppms_mem_attn's p_format / ppms_epilogue.vt_f16 (include/ppms.h)."""
    fmt = TUNING["attn_p"]
    if fmt not in ("fp16", "bf16"):
        raise ValueError(f"TUNING['attn_p'] must be 'fp16' or 'bf16', got {fmt!r}")
    return L.ATTN_P_FP16 if fmt == "fp16" else L.ATTN_P_BF16


# ------------------------------------------------------------------------------------------------ launches
def _timed(fn, events):
    """fn() bracketed by HIP events on the launch stream when bench.py asks for them."""
    if events is not None and KERNEL_TIMING["on"]:
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        pair[0].record()
        fn()
        pair[1].record()
        events.append(pair)
    else:
        fn()


class ConvOp:
    """One implicit-GEMM launch: host descriptor (validated by the library) + its device copy."""

    def __init__(self, desc: L.Conv, keep: list, version: int = CONV2, wm_hint: int = 0, nslice: Optional[int] = None, ysweep: bool = False,
                 device=None):
        self.desc, self.version, self.wm_hint, self.ysweep = desc, int(version), wm_hint, ysweep
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dev = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).clone().to(device)
        self.keep = keep            # tensors whose storage the descriptor points at
        self.events = None          # list collecting (start, stop) HIP events per launch when kernel timing is on
        lib, ref = L.load(), C.byref(desc)
        self._kernel = k = kernel_record(self.version, ysweep)
        # small maps: K-sliced launch + reduce kernel (nslice None: ask the library; own workspace per op because ops
        # of the two streams run concurrently; conv_gemm5's sliced form has the same workspace layout as conv_gemm2's)
        self.nslice, self.ws = k.slices(lib, ref, wm_hint, nslice), None
        if self.nslice > 1:
            self.ws = torch.empty(int(lib.ppms_conv_gemm2_slice_workspace_bytes(ref, self.nslice)), dtype=torch.uint8, device=device)
        # the entry point and every argument but the stream, resolved once: the small scales are chains of short launches
        self._fn, self._args = k.bind(lib, ref, self.dev.data_ptr(), wm_hint, self.nslice, L.ptr(self.ws))

    def flops(self) -> float:
        """Algorithmic FLOPs of one launch: 2 * pixels * stored couts * input channels of the launch * taps (zero-padding
        taps included, as a FLOP counter on the reference conv would)."""
        d = self.desc
        cout = d.epi[0].n_valid + (d.epi[1].n_valid if d.m_split < d.M else 0)
        cin = d.seg[0].c if d.groups == 2 else sum(d.seg[i].c for i in range(d.nseg))       # (grouped: every cout reads its own segment only)
        return 2.0 * d.T * d.H * d.W * cout * cin * d.kt * d.kh * d.kw

    def mfma_per_product(self) -> float:
        """MFMAs the kernel issues per algorithmic bf16x3 product: 3 (hi*hi, lo*hi, hi*lo), less the hi*lo products conv_gemm5 / conv_gemm6 leave out for the
        input channels from `lo_zero_from` on (bf16-exact activations: their lo plane is all zero).  bench.py prices a launch against
        dense bf16 / this."""
        d, k = self.desc, self._kernel
        cin = sum(d.seg[i].c for i in range(d.nseg))
        lz = int(d.lo_zero_from)
        if not k.lo_steps or lz <= 0 or lz >= cin or lz % k.granule:
            return 3.0
        # conv_gemm6's K loop runs the windows with a lo plane first (phase 0) and needs an EVEN number of k32-steps there (its weight registers
        # alternate between two stages): plan6 (conv_gemm6.hip) ignores lo_zero_from when (lo_zero_from / 32) * (k32-steps per window) is odd
        nsweep = d.kh * d.kw if (d.kh > 1 or d.kw > 1) else 1
        if ((lz // k.granule) * nsweep) % k.lo_steps:
            return 3.0
        return 3.0 - (cin - lz) / cin

    def __call__(self):
        _timed(self._launch, self.events)

    def _launch(self):
        L.check(self._fn(*self._args, L.stream_ptr()))


def epilogue(kind=L.EPI_STORE, act=L.ACT_NONE, scale=1.0, n_valid=0, out_sp: Optional[L.SP] = None, out_f32=None, out_f32_ld=0,
             out_vt=None, aux_sp: Optional[L.SP] = None, aux_f32=None, aux_f32_ld=0, pre_f32=None, pre_off=0, vt_f16=None) -> L.Epilogue:
    e = L.Epilogue()
    e.kind, e.act, e.scale, e.n_valid = kind, act, scale, n_valid
    if out_sp is not None:
        e.out_sp = out_sp
    e.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    e.out_f32_ld = out_f32_ld
    e.out_vt = None if out_vt is None else out_vt.data_ptr()
    e.vt_f16 = attn_p_format() if vt_f16 is None else int(vt_f16)      # (only read with out_vt)
    if aux_sp is not None:
        e.aux_sp = aux_sp
    e.aux_f32 = None if aux_f32 is None else aux_f32.data_ptr()
    e.aux_f32_ld = aux_f32_ld
    if pre_f32 is not None:                  # (P, ld) fp32, this half's columns start at pre_off
        e.pre_f32, e.pre_f32_ld = pre_f32.data_ptr() + 4 * pre_off, pre_f32.shape[1]
    return e


class TimedCall:
    """A small-kernel launch (python callable) that bench.py can bracket with HIP events like a ConvOp."""

    def __init__(self, fn):
        self.fn, self.events = fn, None

    def __call__(self):
        _timed(self.fn, self.events)


class PwChain:
    """One fused per-pixel layer chain launch (pwchain.hip): host parameter block + device copy."""

    def __init__(self, inp: L.SP, out: L.SP, layers, pixels: int, keep: list, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        cp = L.ChainParams()
        cp.inp, cp.out, cp.nlayers, cp.P = inp, out, len(layers), pixels
        # (pwchain.hip keeps two activation buffers: the residual operand = the chain input survives only up to the second layer)
        assert not any(resid for _, _, resid, _ in layers[2:]), "pwchain: a residual layer must be the first or the second of its chain"
        for i, (pack, n_valid, resid, post) in enumerate(layers):
            packed, bias, meta = pack
            assert meta["nk"] == 2 and meta["kernel"] == CONV2,"chain layers are 1x1 convs with 64 (padded) input channels"
            ly = cp.layer[i]
            ly.w, ly.bias, ly.M, ly.n_valid, ly.resid = packed.data_ptr(), bias.data_ptr(), meta["M"], n_valid, int(resid)
            ly.post_s = None if post is None else post[0].data_ptr()
            ly.post_t = None if post is None else post[1].data_ptr()
            keep += [packed, bias]
        self.pixels, self.keep, self.cp = pixels, keep, cp
        self.dev = torch.frombuffer(bytearray(bytes(cp)), dtype=torch.uint8).clone().to(device)
        self.events = None

    def __call__(self):
        _timed(lambda: L.check(L.load().ppms_pwchain(self.dev.data_ptr(), self.pixels, L.stream_ptr())), self.events)


# ------------------------------------------------------------------------------------------------ the kernels
class _Shape(NamedTuple):
    """What decides which packs pack_conv builds for a weight."""
    taps: tuple         # (kt, kh, kw)
    pads: list          # padded input channels per segment
    rows: int           # output rows in use
    m2: int             # conv_gemm2's padded rows (gemm1 / conv_stream use the same)

    @property
    def swept(self) -> bool:
        return self.taps[1] > 1 or self.taps[2] > 1

    @property
    def k32(self) -> bool:
        return all(p % 32 == 0 for p in self.pads)

    @property
    def m_waves(self) -> int:
        """conv_gemm5 / conv_gemm6 deal 128, 192 (three 64-cout blocks: convc2's 192, final_conv's 190 couts) or 256 rows to their waves"""
        return 128 if self.rows <= 128 else (192 if self.rows <= 192 else 256)


def _rows_conv6(s: _Shape) -> Optional[int]:
    # conv_gemm6 without a spatial sweep: its STREAM form, for the (kt,1,1) convs to 256 couts (the z/r conv of the GRU's pass T: 131 us against
    # conv_gemm5's 155 at the 1/4 scale; the 128-cout q conv stays on conv_gemm2: 85 us against 89 there)
    return s.m_waves if s.k32 and (s.swept or (s.taps[0] > 1 and s.rows > 128)) else None


def _rows_conv5(s: _Shape) -> Optional[int]:
    if s.swept:
        return s.m_waves
    # no spatial sweep: conv_gemm5's GEMM mode (windows of 64 channels), for > 128 couts only (GRU pass-T z/r 197 -> 164 us, mask_2d.2 62 -> 46 us
    # at the 1/4 scale); with 128 couts the two K-groups get 32-channel windows, too short a DMA lookahead (pass-T q 110 -> 122 us, to_v 44 -> 66 us)
    return (s.rows + 127) // 128 * 128 if s.rows > 128 and s.k32 else None


def _fills_half(d: L.Conv) -> bool:
    """The stored couts fill more than half of the padded rows."""
    return 2 * (d.epi[0].n_valid + (d.epi[1].n_valid if d.m_split < d.M else 0)) > d.M


def _slices_conv2(plan: str):
    """conv_gemm2's K slices: the library's plan (grid-level slicing of the small maps' convs) or the caller's; none under a tile hint."""
    return lambda lib, ref, wm_hint, nslice: 1 if wm_hint != 0 else (max(1, int(getattr(lib, plan)(ref))) if nslice is None else nslice)


class Kernel(NamedTuple):
    """One conv kernel as pack_conv, plan_conv and ConvOp see it."""
    key: object             # pack key: the id, or CONV2_SWEPT
    id: int                 # ConvOp.version
    name: str
    layout: Callable        # packing.py: (weight, bias, segs, seg_pad, cout_map, m) -> (packed, bias, meta)
    granule: int            # input channels per k-step
    swept: bool             # reads its taps in sweep_order
    rows: Callable          # _Shape -> padded rows of the pack pack_conv builds, None: no pack for this weight
    accepts: Callable       # (lib, descriptor with this pack) -> plan_conv launches it here
    bind: Callable          # (lib, ref, dev, wm_hint, nslice, ws) -> (entry point, arguments before the stream)
    slices: Callable = lambda lib, ref, wm_hint, nslice: 1     # -> K slices of the launch
    lo_steps: int = 0       # skips the hi*lo products from ppms_conv.lo_zero_from on when the k-steps before it are a multiple of this (0: never)

    @property
    def ysweep(self) -> bool:
        return self.key == CONV2_SWEPT


# In planning order: plan_conv takes the first whose pack exists and which accepts the descriptor.
KERNELS = (
    # 1x1 convs / Linear layers where the thin GEMM is rated faster (2: served, but the implicit GEMM is as fast on a map this large)
    Kernel(GEMM1, GEMM1, "gemm1", _packing.pack_gemm1, 16, False,
           rows=lambda s: s.m2 if s.taps == (1, 1, 1) and sum(s.pads) % 64 == 0 else None,
           accepts=lambda lib, d: lib.ppms_gemm1_applicable(C.byref(d)) == 1,
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_gemm1, (ref, dev, wm_hint))),
    # small maps (1/8, 1/16 scales): the register-streamed kernel where the library rates it faster -- no K slices, no reduce launch
    Kernel(STREAM, STREAM, "conv_stream", _packing.pack_stream, 16, False,
           rows=lambda s: s.m2 if sum(s.pads) % 64 == 0 else None,
           accepts=lambda lib, d: lib.ppms_conv_stream_applicable(C.byref(d)) == 1,
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_conv_stream, (ref, dev, wm_hint))),
    # conv_gemm6 (one wave per SIMD on the 16x16x32 MFMA) where the library rates its tile fill -- not for couts filling only half of the padded
    # rows (convf2's 64 of 128: 50 us instead of 63 + 117 us of K-sliced launch + reduce, but on the side stream it takes whole CUs from convc2:
    # 35.5 vs 35.4 ms per clip)
    Kernel(CONV6, CONV6, "conv_gemm6", _packing.pack_conv6, 32, True, _rows_conv6, lo_steps=2,
           accepts=lambda lib, d: _fills_half(d) and lib.ppms_conv_gemm6_applicable(C.byref(d)) == 1,
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_conv_gemm6, (ref, dev))),
    # conv_gemm5 (one 8-wave workgroup per CU, weights in MFMA-fragment order) where it serves the map, same fill rule (convf2 on it: 78 us instead
    # of 65 + 143 us, clip time unchanged, 40.8 ms); K-sliced only on the caller's request
    Kernel(CONV5, CONV5, "conv_gemm5", _packing.pack_conv5, 16, True, _rows_conv5, lo_steps=1,
           accepts=lambda lib, d: _fills_half(d) and bool(lib.ppms_conv_gemm5_applicable(C.byref(d))),
           slices=lambda lib, ref, wm_hint, nslice: int(nslice) if nslice is not None and nslice > 1 else 1,
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_conv_gemm5_sliced, (ref, dev, wm_hint, nslice, ws)) if nslice > 1 else
                                                            (lib.ppms_conv_gemm5, (ref, dev, wm_hint))),
    # (kt, kh, 1) convs the faster kernels do not take: conv_gemm2 with one y-swept window for all taps of a (dt, chunk), when the halo'd window fits
    Kernel(CONV2_SWEPT, CONV2, "conv_gemm2", _packing.pack_conv2, 32, True,
           rows=lambda s: s.m2 if s.taps[1] > 1 and s.taps[2] == 1 else None,
           accepts=lambda lib, d: d.kh > 1 and d.kw == 1 and lib.ppms_conv_gemm2_ysweep_slices(C.byref(d)) > 0,
           slices=_slices_conv2("ppms_conv_gemm2_ysweep_slices"),
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_conv_gemm2_ysweep, (ref, dev, nslice, ws))),
    # conv_gemm2 (implicit GEMM through LDS) serves every conv: always packed, optionally K-sliced (+ a reduce launch)
    Kernel(CONV2, CONV2, "conv_gemm2", _packing.pack_conv2, 32, False,
           rows=lambda s: s.m2,
           accepts=lambda lib, d: True,
           slices=_slices_conv2("ppms_conv_gemm2_slices"),
           bind=lambda lib, ref, dev, wm_hint, nslice, ws: (lib.ppms_conv_gemm2_sliced, (ref, dev, nslice, ws)) if nslice > 1 else
                                                            (lib.ppms_conv_gemm2, (ref, dev, wm_hint))),
)
_BY_KEY = {k.key: k for k in KERNELS}
KERNEL_NAMES = {k.id: k.name for k in KERNELS}
ALL_KERNELS = frozenset(_BY_KEY)


def kernel_record(version: int, ysweep: bool = False) -> Kernel:
    """The record a ConvOp of this version launches through (ysweep: conv_gemm2's one-window form; no other kernel has one)."""
    k = _BY_KEY[version]
    return _BY_KEY[CONV2_SWEPT] if ysweep and k is _BY_KEY[CONV2] else k


# ------------------------------------------------------------------------------------------------ packing
def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def sweep_taps(kt: int, kh: int, kw: int) -> tuple:
    """The tap shape of a sweep-ordered (kt, kh, kw) weight: the LAST axis is the swept one."""
    return (kt, 1, kh * kw) if kh > 1 and kw > 1 else ((kt, kw, kh) if kh > 1 else (kt, kh, kw))


def sweep_order(w5: torch.Tensor) -> torch.Tensor:
    """A (cout, cin, kt, kh, kw) weight in the k-step order of the kernels that sweep one window per tap row (conv_gemm5, conv_gemm6 and
    conv_gemm2's one-window form): the LAST kernel axis is the swept one -- y sweep: kh / kw swapped; 2-D sweep: (ky, kx) flattened into x."""
    co, ci, kt, kh, kw = w5.shape
    if kh > 1 and kw > 1:
        return w5.reshape(co, ci, kt, 1, kh * kw).contiguous()
    if kh > 1:
        return w5.transpose(3, 4).contiguous()
    return w5


def sweep_inverse(ws: torch.Tensor, taps) -> torch.Tensor:
    """sweep_order undone: a (cout, cin, *sweep_taps(*taps)) weight back in its natural (cout, cin, kt, kh, kw) order."""
    kt, kh, kw = taps
    if kh > 1 and kw > 1:
        return ws.reshape(*ws.shape[:2], kt, kh, kw)
    if kh > 1:
        return ws.transpose(3, 4)
    return ws


def pack_for(kernel, weight: torch.Tensor, bias: Optional[torch.Tensor], segs: Sequence[int], seg_pad: Optional[Sequence[int]] = None,
             cout_map: Optional[Sequence[int]] = None, m: Optional[int] = None) -> tuple:
    """ONE kernel's pack (packed, bias, meta) of a 4-D / 5-D weight: the layout function of packing.py, on the sweep-ordered weight for the
    swept kernels.  m: the padded cout rows (None: the layout's own default)."""
    k = _BY_KEY[kernel]
    if k.swept:
        weight = sweep_order(weight if weight.dim() == 5 else weight[:, :, None])
    return k.layout(weight, bias, segs, seg_pad, cout_map, m)


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], segs: Sequence[int], seg_pad: Optional[Sequence[int]] = None,
              cout_map: Optional[Sequence[int]] = None, m_pad: Optional[int] = None, kernels=ALL_KERNELS) -> Dict[object, tuple]:
    """kernel -> (packed, bias, meta) of every kernel in `kernels` that can serve a conv of this weight (2-D Linear (cout, cin), 4-D Conv2d or
    5-D Conv3d), and always conv_gemm2's.  segs: input channels per segment, each zero-padded to seg_pad (default: a multiple of 32);
    cout_map: the output row of each cout; m_pad: conv_gemm2's padded rows (gemm1 / conv_stream use the same)."""
    if weight.dim() == 2:
        weight = weight[:, :, None, None]
    w5 = weight if weight.dim() == 5 else weight[:, :, None]
    pads = list(seg_pad) if seg_pad is not None else [_pad32(c) for c in segs]
    rows = (max(cout_map) + 1) if cout_map is not None else w5.shape[0]
    shape = _Shape(tuple(w5.shape[2:]), pads, rows, (rows + 63) // 64 * 64 if m_pad is None else m_pad)
    packs = {}
    for k in KERNELS:
        m = k.rows(shape) if (k.key in kernels or k is _BY_KEY[CONV2]) else None
        if m is not None:
            packs[k.key] = pack_for(k.key, weight, bias, segs, pads, cout_map, m)
    return packs


# ------------------------------------------------------------------------------------------------ planning
def conv_desc(segs: Sequence[L.SP], thw, taps, epi0: L.Epilogue, epi1: Optional[L.Epilogue] = None, m_split: int = 0, t_halo: int = 0,
              lo_zero_from: int = 0) -> L.Conv:
    """A descriptor without weights: input segments, (T, H, W), taps, epilogue halves (m_split 0: one half over every row), the temporal
    halo slabs and the first bf16-exact input channel (ppms_conv.lo_zero_from: a promise, see ppms.h).  plan_conv fills in the pack."""
    d = L.Conv()
    for i, s in enumerate(segs):
        d.seg[i] = s
    d.nseg = len(segs)
    d.T, d.H, d.W = thw
    d.kt, d.kh, d.kw = taps
    d.m_split, d.t_halo, d.lo_zero_from = m_split, t_halo, lo_zero_from
    d.epi[0] = epi0
    if epi1 is not None:
        d.epi[1] = epi1
    return d


def _with_pack(desc: L.Conv, pack: tuple, keep) -> tuple:
    packed, bias, meta = pack
    d = L.Conv.from_buffer_copy(bytes(desc))
    d.w, d.bias, d.M = packed.data_ptr(), bias.data_ptr(), meta["M"]
    if desc.m_split == 0:
        d.m_split = meta["M"]
    return d, [packed, bias, *keep]


def plan_conv(desc: L.Conv, packs: Dict[object, tuple], keep=(), nslice: Optional[int] = None, device=None) -> Optional[ConvOp]:
    """The launch of `desc` (conv_desc) on the first kernel (in the order of KERNELS) whose pack exists and which accepts it.  None when no
    pack serves it (a caller without a conv_gemm2 pack).  nslice: conv_gemm2's K slices (None: the library's plan)."""
    lib = L.load()
    if CONV2 in packs:
        meta = packs[CONV2][2]
        assert [desc.seg[i].c for i in range(desc.nseg)] == meta["seg_padded"], ([desc.seg[i].c for i in range(desc.nseg)], meta["seg_padded"])
        assert (desc.kt, desc.kh, desc.kw) == meta["taps"], ((desc.kt, desc.kh, desc.kw), meta["taps"])
    for k in KERNELS:
        if k.key in packs:
            d, kept = _with_pack(desc, packs[k.key], keep)
            if k.accepts(lib, d):
                return ConvOp(d, kept, k.id, nslice=nslice if k is _BY_KEY[CONV2] else None, ysweep=k.ysweep, device=device)
    return None
