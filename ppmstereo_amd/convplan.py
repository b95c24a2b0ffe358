"""Which HIP kernel runs a convolution, and the weight packs it reads: the one place where every engine (the update block's ScaleEngine,
fnet, cnet, the SST block) packs its conv weights and plans its launches.

A convolution is packed once (``pack_conv``: one pack per kernel the caller allows and the weight's shape suits) and planned once per
geometry (``plan_conv``: the first kernel, in a fixed order, whose pack exists and which the library rates for the descriptor).  The
result is a ``ConvOp``: the host descriptor, its device copy and the resolved entry point, launched on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L
from . import packing as _packing

# Kernel identities (ConvOp.version; bench.py and the tests read the plain ints)
CONV2 = 2           # conv_gemm2.hip: implicit GEMM through LDS, optionally K-sliced (+ a reduce launch)
CONV5 = 5           # conv_gemm5.hip: one 8-wave workgroup per CU, weights in MFMA-fragment order
GEMM1 = 6           # gemm1.hip: thin GEMM of the 1x1 convolutions / Linear layers
STREAM = 7          # conv_stream.hip: register-streamed small-map kernel (no K slices, no reduce launch)
CONV6 = 8           # conv_gemm6.hip: one wave per SIMD on the 16x16x32 MFMA
CONV2_SWEPT = "2s"  # (pack key only) conv_gemm2's one-window form: the swept weight order of a (kt, kh, 1) conv, launched as CONV2 with ysweep
KERNEL_NAMES = {CONV2: "conv_gemm2", CONV5: "conv_gemm5", GEMM1: "gemm1", STREAM: "conv_stream", CONV6: "conv_gemm6"}
ALL_KERNELS = frozenset((CONV2, CONV2_SWEPT, CONV5, GEMM1, STREAM, CONV6))

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
        # small maps: K-sliced launch + reduce kernel (nslice None: ask the library; own workspace per op because ops
        # of the two streams run concurrently)
        self.nslice, self.ws = 1, None
        if version == CONV5 and nslice is not None and nslice > 1:      # conv_gemm5's K-sliced form (same workspace layout as conv_gemm2's)
            self.nslice = int(nslice)
        elif version == CONV2 and wm_hint == 0:
            plan = lib.ppms_conv_gemm2_ysweep_slices if ysweep else lib.ppms_conv_gemm2_slices
            self.nslice = max(1, int(plan(ref))) if nslice is None else nslice
        if self.nslice > 1:
            self.ws = torch.empty(int(lib.ppms_conv_gemm2_slice_workspace_bytes(ref, self.nslice)), dtype=torch.uint8, device=device)
        # the entry point and every argument but the stream, resolved once: the small scales are chains of short launches
        dp, ws = self.dev.data_ptr(), L.ptr(self.ws)
        if version == CONV5 and self.nslice > 1:
            self._fn, self._args = lib.ppms_conv_gemm5_sliced, (ref, dp, wm_hint, self.nslice, ws)
        elif version == CONV5:
            self._fn, self._args = lib.ppms_conv_gemm5, (ref, dp, wm_hint)
        elif version == CONV6:
            self._fn, self._args = lib.ppms_conv_gemm6, (ref, dp)
        elif version == GEMM1:
            self._fn, self._args = lib.ppms_gemm1, (ref, dp, wm_hint)
        elif version == STREAM:
            self._fn, self._args = lib.ppms_conv_stream, (ref, dp, wm_hint)
        elif ysweep:
            self._fn, self._args = lib.ppms_conv_gemm2_ysweep, (ref, dp, self.nslice, ws)
        elif self.nslice > 1:
            self._fn, self._args = lib.ppms_conv_gemm2_sliced, (ref, dp, self.nslice, ws)
        else:
            self._fn, self._args = lib.ppms_conv_gemm2, (ref, dp, wm_hint)

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
        d = self.desc
        cin = sum(d.seg[i].c for i in range(d.nseg))
        lz = int(d.lo_zero_from)
        if self.version not in (CONV5, CONV6) or lz <= 0 or lz >= cin or lz % (16 if self.version == CONV5 else 32):
            return 3.0
        if self.version == CONV6:
            # conv_gemm6's K loop runs the windows with a lo plane first (phase 0) and needs an EVEN number of k32-steps there (its weight registers
            # alternate between two stages): plan6 (conv_gemm6.hip) ignores lo_zero_from when (lo_zero_from / 32) * (k32-steps per window) is odd
            nsweep = d.kh * d.kw if (d.kh > 1 or d.kw > 1) else 1
            if ((lz // 32) * nsweep) & 1:
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
            assert meta["nk"] == 2 and meta["version"] == 2, "chain layers are 1x1 convs with 64 (padded) input channels"
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


# ------------------------------------------------------------------------------------------------ packing
def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def sweep_order(w5: torch.Tensor) -> torch.Tensor:
    """A (cout, cin, kt, kh, kw) weight in the k-step order of the kernels that sweep one window per tap row (conv_gemm5, conv_gemm6 and
    conv_gemm2's one-window form): the LAST kernel axis is the swept one -- y sweep: kh / kw swapped; 2-D sweep: (ky, kx) flattened into x."""
    co, ci, kt, kh, kw = w5.shape
    if kh > 1 and kw > 1:
        return w5.reshape(co, ci, kt, 1, kh * kw).contiguous()
    if kh > 1:
        return w5.transpose(3, 4).contiguous()
    return w5


def pack_for(kernel, weight: torch.Tensor, bias: Optional[torch.Tensor], segs: Sequence[int], seg_pad: Optional[Sequence[int]] = None,
             cout_map: Optional[Sequence[int]] = None, m: Optional[int] = None) -> tuple:
    """ONE kernel's pack (packed, bias, meta) of a 4-D / 5-D weight: the layout function of packing.py, on the sweep-ordered weight for the
    swept kernels.  m: the padded cout rows (None: the layout's own default)."""
    w5 = weight if weight.dim() == 5 else weight[:, :, None]
    if kernel in (CONV5, CONV6, CONV2_SWEPT) and (w5.shape[3] > 1 or w5.shape[4] > 1):
        weight = sweep_order(w5)
    fn = {CONV2: _packing.pack_conv2, CONV2_SWEPT: _packing.pack_conv2, CONV5: _packing.pack_conv4, CONV6: _packing.pack_conv6,
          GEMM1: _packing.pack_gemm1, STREAM: _packing.pack_stream}[kernel]
    return fn(weight, bias, segs, seg_pad, cout_map, m)


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], segs: Sequence[int], seg_pad: Optional[Sequence[int]] = None,
              cout_map: Optional[Sequence[int]] = None, m_pad: Optional[int] = None, kernels=ALL_KERNELS) -> Dict[object, tuple]:
    """kernel -> (packed, bias, meta) of every kernel in `kernels` that can serve a conv of this weight (2-D Linear (cout, cin), 4-D Conv2d or
    5-D Conv3d).  segs: input channels per segment, each zero-padded to seg_pad (default: a multiple of 32); cout_map: the output row of each
    cout; m_pad: conv_gemm2's padded rows (gemm1 / conv_stream use the same)."""
    if weight.dim() == 2:
        weight = weight[:, :, None, None]
    w5 = weight if weight.dim() == 5 else weight[:, :, None]
    kt, kh, kw = w5.shape[2:]
    pads = list(seg_pad) if seg_pad is not None else [_pad32(c) for c in segs]
    rows = (max(cout_map) + 1) if cout_map is not None else w5.shape[0]
    packs = {CONV2: pack_for(CONV2, weight, bias, segs, pads, cout_map, m_pad)}
    m2 = packs[CONV2][2]["M"]
    if GEMM1 in kernels and (kt, kh, kw) == (1, 1, 1) and sum(pads) % 64 == 0:
        packs[GEMM1] = pack_for(GEMM1, weight, bias, segs, pads, cout_map, m2)
    if STREAM in kernels and sum(pads) % 64 == 0:
        packs[STREAM] = pack_for(STREAM, weight, bias, segs, pads, cout_map, m2)
    if CONV2_SWEPT in kernels and kh > 1 and kw == 1:
        packs[CONV2_SWEPT] = pack_for(CONV2_SWEPT, weight, bias, segs, pads, cout_map, m_pad)
    # conv_gemm5 / conv_gemm6 deal 128, 192 (three 64-cout blocks: convc2's 192, final_conv's 190 couts) or 256 rows to their waves
    m = 128 if rows <= 128 else (192 if rows <= 192 else 256)
    swept, k32 = kh > 1 or kw > 1, all(p % 32 == 0 for p in pads)
    # conv_gemm6 without a spatial sweep: its STREAM form, for the (kt,1,1) convs to 256 couts (the z/r conv of the GRU's pass T: 131 us against
    # conv_gemm5's 155 at the 1/4 scale; the 128-cout q conv stays on conv_gemm2: 85 us against 89 there)
    if CONV6 in kernels and k32 and (swept or (kt > 1 and rows > 128)):
        packs[CONV6] = pack_for(CONV6, weight, bias, segs, pads, cout_map, m)
    if CONV5 in kernels and swept:
        packs[CONV5] = pack_for(CONV5, weight, bias, segs, pads, cout_map, m)
    elif CONV5 in kernels and rows > 128 and k32:
        # no spatial sweep: conv_gemm5's GEMM mode (windows of 64 channels), for > 128 couts only (GRU pass-T z/r 197 -> 164 us, mask_2d.2 62 -> 46 us
        # at the 1/4 scale); with 128 couts the two K-groups get 32-channel windows, too short a DMA lookahead (pass-T q 110 -> 122 us, to_v 44 -> 66 us)
        packs[CONV5] = pack_for(CONV5, weight, bias, segs, pads, cout_map, (rows + 127) // 128 * 128)
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


def _fills_half(d: L.Conv) -> bool:
    """The stored couts fill more than half of the padded rows."""
    return 2 * (d.epi[0].n_valid + (d.epi[1].n_valid if d.m_split < d.M else 0)) > d.M


def plan_conv(desc: L.Conv, packs: Dict[object, tuple], keep=(), nslice: Optional[int] = None, device=None) -> Optional[ConvOp]:
    """The launch of `desc` (conv_desc) on the first kernel whose pack exists and which the library rates for it.  None when no pack serves
    it (a caller without a conv_gemm2 pack).  nslice: conv_gemm2's K slices (None: the library's plan)."""
    lib = L.load()
    if CONV2 in packs:
        meta = packs[CONV2][2]
        assert [desc.seg[i].c for i in range(desc.nseg)] == meta["seg_padded"], ([desc.seg[i].c for i in range(desc.nseg)], meta["seg_padded"])
        assert (desc.kt, desc.kh, desc.kw) == meta["taps"], ((desc.kt, desc.kh, desc.kw), meta["taps"])
    # 1. 1x1 convs where the thin GEMM is rated faster (2: served, but the implicit GEMM is as fast on a map this large)
    if GEMM1 in packs:
        d, k = _with_pack(desc, packs[GEMM1], keep)
        if lib.ppms_gemm1_applicable(C.byref(d)) == 1:
            return ConvOp(d, k, GEMM1, device=device)
    # 2. small maps (1/8, 1/16 scales): the register-streamed kernel where the library rates it faster -- no K slices, no reduce launch
    if STREAM in packs:
        d, k = _with_pack(desc, packs[STREAM], keep)
        if lib.ppms_conv_stream_applicable(C.byref(d)) == 1:
            return ConvOp(d, k, STREAM, device=device)
    # 3. conv_gemm6 where the library rates its tile fill -- not for couts filling only half of the padded rows (convf2's 64 of 128: 50 us instead
    #    of 63 + 117 us of K-sliced launch + reduce, but on the side stream it takes whole CUs from convc2: 35.5 vs 35.4 ms per clip)
    if CONV6 in packs:
        d, k = _with_pack(desc, packs[CONV6], keep)
        if _fills_half(d) and lib.ppms_conv_gemm6_applicable(C.byref(d)) == 1:
            return ConvOp(d, k, CONV6, device=device)
    # 4. conv_gemm5 where it serves the map, same fill rule (convf2 on it: 78 us instead of 65 + 143 us, clip time unchanged, 40.8 ms)
    if CONV5 in packs:
        d, k = _with_pack(desc, packs[CONV5], keep)
        if _fills_half(d) and lib.ppms_conv_gemm5_applicable(C.byref(d)):
            return ConvOp(d, k, CONV5, device=device)
    # 5. (kt, kh, 1) convs the faster kernels do not take: conv_gemm2 with one y-swept window for all taps of a (dt, chunk), when the halo'd window fits
    if CONV2_SWEPT in packs and desc.kh > 1 and desc.kw == 1:
        d, k = _with_pack(desc, packs[CONV2_SWEPT], keep)
        if lib.ppms_conv_gemm2_ysweep_slices(C.byref(d)) > 0:
            return ConvOp(d, k, CONV2, ysweep=True, device=device)
    # 6. conv_gemm2: the library's K-slice plan (grid-level slicing of the small maps' convs) or the caller's
    if CONV2 in packs:
        d, k = _with_pack(desc, packs[CONV2], keep)
        return ConvOp(d, k, CONV2, nslice=nslice, device=device)
    return None
