"""The hot loop with the reference's call signature, and the thin caller-side glue needed to drive it.

``forward_update_block`` keeps the signature and side effects of
``PPMStereo.forward_update_block`` (/root/reference/models/core/ppmstereo.py:426-594): it can be bound as a method
of the reference's ``PPMStereo`` or used through ``PPMStereoHotPath`` below, which also holds
the three update blocks / q-k projections under the reference's attribute names (``update_block16/08/04``,
``att``) so a reference checkpoint loads with ``strict=False``.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .corr import CorrBlock1D
from .engine import bilinear
from .update import Attention_qk, SequenceUpdateBlock3D


def interp(x: torch.Tensor, size) -> torch.Tensor:
    """models/core/utils/utils.py:10-16 (bilinear, align_corners=True)."""
    return bilinear(x, (int(size[0]), int(size[1])), True)


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor, rate: int = 4) -> torch.Tensor:
    """PPMStereo.convex_upsample, ppmstereo.py:185-197 (NCHW in, NCHW out)."""
    if rate != 4:
        raise NotImplementedError("convex_upsample: rate 4 only")
    L.require_gpu(flow, mask)
    N, _, H, W = flow.shape
    lib, s = L.load(), L.stream_ptr()
    f = torch.empty(N * H * W, 2, dtype=torch.float32, device=flow.device)
    m = torch.empty(N * H * W, 144, dtype=torch.float32, device=flow.device)
    fc, mc = flow.contiguous().float(), mask.contiguous().float()
    L.check(lib.ppms_nchw_to_nhwc(fc.data_ptr(), f.data_ptr(), 2, N, 2, H * W, s))
    L.check(lib.ppms_nchw_to_nhwc(mc.data_ptr(), m.data_ptr(), 144, N, 144, H * W, s))
    out = torch.empty(N, 2, 4 * H, 4 * W, dtype=torch.float32, device=flow.device)
    L.check(lib.ppms_convex_upsample(f.data_ptr(), m.data_ptr(), 144, out.data_ptr(), N, H, W, s))
    return out


def _run_iterations(eng, iters: int, isc: int, t: int, h: int, w: int, predictions: List, uncertainties: List, emit: str = "all"):
    """The iteration loop on a prepared engine (ppmstereo.py:482-591).  emit: which iterations resize their prediction and
    uncertainty to full resolution and append them (:578-591): "all" (the reference's lists), "last" or "none" --
    PPMStereo.forward(test_mode=True) returns predictions[-1] alone (:801-804), so every other resize is dead work there."""
    flow_out = None
    for it in range(iters):
        # the upsampled flow of an iteration is consumed by its prediction (when emitted) and, after the last iteration, by the next
        # scale's initialisation (:724-725): anywhere else the mask head + convex upsampling are dead work and are not launched
        flow_out = eng.iterate(need_up=(emit == "all" or it + 1 == iters))
        if emit == "none" or (emit == "last" and it + 1 < iters):
            continue
        unc_up = bilinear(eng.UNC_local().view(t, 1, h, w), (4 * isc * h, 4 * isc * w), False)
        if isc > 1:
            flow_up = bilinear(flow_out[:, :1], (isc * 4 * h, isc * 4 * w), True, float(isc))
        else:
            flow_up = flow_out[:, :1].clone()
        predictions.append(flow_up)
        uncertainties.append(unc_up)
    return flow_out


def _add_attn_redo(diagnostics: dict, per_scale: Dict[str, Dict[str, int]]):
    """diagnostics["attn_redo"][scale][counter] += per_scale[scale][counter] (entries already present are kept: a caller sums over windows)."""
    total = diagnostics.setdefault("attn_redo", {})
    for tag, counters in per_scale.items():
        entry = total.setdefault(tag, {"calls": 0, "tiles": 0, "flagged": 0})
        for k, v in counters.items():
            entry[k] += int(v)


def convex_upsample_3d(flow: torch.Tensor, mask: torch.Tensor, rate: int, T: int) -> torch.Tensor:
    """PPMStereo.convex_upsample_3d, ppmstereo.py:199-228 (NCHW in, NCHW out; one window of T frames, batch 1)."""
    if rate != 4:
        raise NotImplementedError("convex_upsample_3d: rate 4 only")
    L.require_gpu(flow, mask)
    N, _, H, W = flow.shape
    if N != T:
        raise NotImplementedError("convex_upsample_3d: batch size 1 (N == T)")
    lib, s = L.load(), L.stream_ptr()
    f = torch.empty(N * H * W, 2, dtype=torch.float32, device=flow.device)
    m = torch.empty(N * H * W, 432, dtype=torch.float32, device=flow.device)
    fc, mc = flow.contiguous().float(), mask.contiguous().float()
    L.check(lib.ppms_nchw_to_nhwc(fc.data_ptr(), f.data_ptr(), 2, N, 2, H * W, s))
    L.check(lib.ppms_nchw_to_nhwc(mc.data_ptr(), m.data_ptr(), 432, N, 432, H * W, s))
    out = torch.empty(N, 2, 4 * H, 4 * W, dtype=torch.float32, device=flow.device)
    L.check(lib.ppms_convex_upsample_3d(f.data_ptr(), m.data_ptr(), 432, out.data_ptr(), T, H, W, 0, s))
    return out


def forward_update_block(self, image1, update_block: SequenceUpdateBlock3D, corr_fn: CorrBlock1D, flow: torch.Tensor, net: torch.Tensor,
                         inp: torch.Tensor, motion_hidden_state: Optional[torch.Tensor], attn_block: Attention_qk, predictions: List,
                         uncertainties: List, iters: int, interp_scale: float, t: int):
    """Same contract as PPMStereo.forward_update_block (ppmstereo.py:426-594): runs ``iters`` refinement
    iterations at one scale, appends one full-resolution prediction and uncertainty per iteration and returns
    (flow_out (BT,2,4h,4w), net (BT,128,h,w), motion_hidden_state (BT,64,h,w)).  ``image1`` is unused (as in the
    reference).  BT = b * t: batch elements are independent except for the normaliser of the frame scores (:533), see
    ``_forward_update_block_batched``; b = 1 (inference) is the device-resident fast path."""
    L.require_gpu(flow, net, inp)
    bt, c, h, w = inp.shape
    if bt % t:
        raise RuntimeError(f"forward_update_block: {bt} frames do not divide into clips of t = {t}")
    if bt != t:
        return _forward_update_block_batched(update_block, corr_fn, flow, net, inp, motion_hidden_state, attn_block, predictions, uncertainties,
                                             iters, interp_scale, t)
    if c != 128:
        raise RuntimeError("forward_update_block: 128 context channels expected")
    if int(interp_scale) not in (1, 2, 4):
        raise NotImplementedError("interp_scale must be 4, 2 or 1 (the reference's only live branches)")
    if t == 1:
        # the reference divides 0/0 in the temporal encoding (ppmtereo_update.py:34-36): every output is NaN
        warnings.warn("PPMStereo with a single frame produces NaN disparities (reference behaviour, T must be >= 2)")
    isc = int(interp_scale)
    with torch.cuda.device(inp.device):         # kernels go to the current stream of the tensors' device
        eng = update_block.engine(t, h, w, inp.device)
        eng.set_inp(inp)
        eng.set_net(net)
        eng.set_flow(flow)
        eng.set_mhs(motion_hidden_state)
        eng.begin(corr_fn.levels, attn_block.packed(inp.device))
        flow_out = _run_iterations(eng, iters, isc, t, h, w, predictions, uncertainties)
        return flow_out.clone(), eng.get_net(), eng.get_mhs()


def _forward_update_block_batched(update_block, corr_fn, flow, net, inp, motion_hidden_state, attn_block, predictions, uncertainties, iters,
                                  interp_scale, t: int):
    """forward_update_block for b > 1 clips in one call (ppmstereo.py:443-449: frame index = bi * t + ti).  Everything is per batch element
    -- the 3-D convolutions, the frame similarity, the top-5 pick and the attention all see one clip -- except ONE scalar per clip index:
    ``selected_score.mean()`` at :533 averages the picked frames' scores over the batch as well, so the key modulation s_hat of clip i is
    its score divided by the mean over all b elements.  One engine per element; the stages run element by element, the normaliser is
    fixed between the pick and the attention."""
    bt, c, h, w = inp.shape
    b = bt // t
    if c != 128 or int(interp_scale) not in (1, 2, 4):
        raise RuntimeError("forward_update_block: 128 context channels and interp_scale 4, 2 or 1 expected")
    if t == 1:
        warnings.warn("PPMStereo with a single frame produces NaN disparities (reference behaviour, T must be >= 2)")
    isc, dev = int(interp_scale), inp.device
    rows = t * h * w
    with torch.cuda.device(dev):
        engs = []
        for bi in range(b):
            sl = slice(bi * t, (bi + 1) * t)
            eng = update_block.engine(t, h, w, dev, slot=bi)
            eng.set_inp(inp[sl]), eng.set_net(net[sl]), eng.set_flow(flow[sl])
            eng.set_mhs(None if motion_hidden_state is None else motion_hidden_state[sl])
            eng.begin([lv[bi * rows:(bi + 1) * rows] for lv in corr_fn.levels], attn_block.packed(dev))      # the pyramid is per frame: row slices
            engs.append(eng)
        k = engs[0].ksel
        flow_out = None
        for _ in range(iters):
            for eng in engs:
                eng.lookup(), eng.motion_and_value(), eng.uncertainty(), eng.pick()
            picked = [eng.SCORE.gather(1, eng.SEL[:, :k].long()) for eng in engs]                            # (t, k) scores of the picked frames
            mean_all = torch.stack([x.sum(1) for x in picked]).sum(0) / float(b * k)                           # :533: the mean runs over the batch too
            outs, uncs = [], []
            for eng, x in zip(engs, picked):
                eng.SHAT[:, :k] = x / mean_all[:, None]
                eng.attend(), eng.update(need_mask=True)
                outs.append(eng.upsample().clone())
                uncs.append(eng.UNC_local().view(t, 1, h, w).clone())
            flow_out = torch.cat(outs)
            unc = torch.cat(uncs)
            uncertainties.append(bilinear(unc, (4 * isc * h, 4 * isc * w), False))
            predictions.append(bilinear(flow_out[:, :1], (isc * 4 * h, isc * 4 * w), True, float(isc)) if isc > 1 else flow_out[:, :1].clone())
        return flow_out, torch.cat([e.get_net() for e in engs]), torch.cat([e.get_mhs() for e in engs])


_PLANE_FORMATS = {"f32": (L.FMT_F32, torch.float32), "f16": (L.FMT_F16, torch.float16), "u16": (L.FMT_U16, torch.uint16), "u8": (L.FMT_U8, torch.uint8)}


class OutputSpec:
    """What ``forward(output=...)`` / ``forward_batch_test(output=...)`` hand back instead of float32 disparity: up to three planes that ONE
    kernel (ppms_disparity_egress, include/ppms.h) writes from the 1/4 scale's last iteration -- crop, kept frames, ``.abs()``, the 4x
    upsampling of the uncertainty and the conversion in one pass.
      disparity    "f32" | "f16" | "u16": d = |disparity| in pixels; "u16" = min(65535, rint(d * disp_scale)) (KITTI: disp_scale = 256), NaN -> 0
      depth        None | "f32" | "f16" | "u16": Z = fb / d with fb = focal_px * baseline (one fp32 product); "u16" = min(65535, rint(Z * depth_scale))
                   (baseline in metres and depth_scale = 1000: millimetres).  A pixel with d < min_disp or d = NaN is invalid: +inf in the float
                   formats, 0 in "u16".  (min_disp = 0 leaves only NaN invalid: d = 0 then gives +inf / 65535.)
      uncertainty  "f32" | "u8" | None: u = |uncertainty| in [0, 1]; "u8" = min(255, rint(u * 255)), NaN -> 0
    Every step is one fp32 operation rounded to nearest even; ``reference`` restates them in torch and is the definition the kernel is
    tested against, bit for bit."""

    def __init__(self, disparity: str = "f32", depth: Optional[str] = None, uncertainty: Optional[str] = "f32", disp_scale: float = 256.0,
                 focal_px: Optional[float] = None, baseline: Optional[float] = None, depth_scale: float = 1000.0, min_disp: float = 2.0 ** -8):
        if disparity not in ("f32", "f16", "u16"):
            raise ValueError(f"OutputSpec: disparity = {disparity!r}; one of 'f32', 'f16', 'u16'")
        if depth not in (None, "f32", "f16", "u16"):
            raise ValueError(f"OutputSpec: depth = {depth!r}; None or one of 'f32', 'f16', 'u16'")
        if uncertainty not in (None, "f32", "u8"):
            raise ValueError(f"OutputSpec: uncertainty = {uncertainty!r}; None, 'f32' or 'u8'")
        f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
        self.disparity, self.depth, self.uncertainty = disparity, depth, uncertainty
        self.disp_scale, self.depth_scale, self.min_disp = f32(disp_scale), f32(depth_scale), f32(min_disp)
        if not (0.0 < self.disp_scale < math.inf):
            raise ValueError(f"OutputSpec: disp_scale = {disp_scale} must be positive and finite")
        self.focal_px, self.baseline, self.fb = focal_px, baseline, 0.0
        if depth is not None:
            if focal_px is None or baseline is None:
                raise ValueError("OutputSpec: a depth plane needs focal_px (focal length in pixels) and baseline")
            self.fb = float(torch.tensor(float(focal_px), dtype=torch.float32) * torch.tensor(float(baseline), dtype=torch.float32))
            if not (0.0 < self.fb < math.inf):
                raise ValueError(f"OutputSpec: focal_px * baseline = {self.fb} must be positive and finite")
            if not (0.0 < self.depth_scale < math.inf):
                raise ValueError(f"OutputSpec: depth_scale = {depth_scale} must be positive and finite")
            if not math.isfinite(self.min_disp):
                raise ValueError(f"OutputSpec: min_disp = {min_disp} must be finite")

    def formats(self) -> Dict[str, str]:
        """{result key: format} of the requested planes, in the order disparity, depth, uncertainties."""
        named = (("disparity", self.disparity), ("depth", self.depth), ("uncertainties", self.uncertainty))
        return {k: f for k, f in named if f is not None}

    def empty(self, n: int, h0: int, w0: int, device, pin_memory: bool = False) -> Dict[str, torch.Tensor]:
        """Dense (n, 1, h0, w0) tensors of the requested planes' dtypes."""
        return {k: torch.empty(n, 1, h0, w0, dtype=_PLANE_FORMATS[f][1], device=device, pin_memory=pin_memory) for k, f in self.formats().items()}

    def struct(self, planes: Dict[str, torch.Tensor]) -> L.Egress:
        """The ``ppms_egress`` that writes into ``planes`` (dense (n, 1, h0, w0) device tensors from ``empty``)."""
        def plane(key):
            t = planes.get(key)
            if t is None:
                return L.EgressPlane(None, 0, 0, 0, 0)
            es = t.element_size()
            return L.EgressPlane(t.data_ptr(), t.stride(0) * es, t.stride(2) * es, _PLANE_FORMATS[self.formats()[key]][0], 0)
        return L.Egress(plane("disparity"), plane("depth"), plane("uncertainties"), self.disp_scale, self.fb, self.depth_scale, self.min_disp)

    def reference(self, d: torch.Tensor, u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The arithmetic of ppms_disparity_egress in plain torch, on CPU or device tensors of any shape: d = a float32 (signed) disparity,
        u = a float32 uncertainty at the same resolution -> the requested planes under forward_batch_test's keys."""
        const = lambda x: torch.full((), x, dtype=torch.float32, device=d.device)

        def quant(v, scale, top, fmt):                       # min(top, rint(v * scale)), NaN -> 0: one fp32 product, ties to even
            r = torch.round(v * const(scale))
            r = torch.where(torch.isnan(r), torch.zeros_like(r), r).clamp(max=top)
            return r.to(torch.int32).to(_PLANE_FORMATS[fmt][1])

        d = d.float().abs()
        out = {"disparity": d if self.disparity == "f32" else d.to(torch.float16) if self.disparity == "f16" else quant(d, self.disp_scale, 65535.0, "u16")}
        if self.depth is not None:
            valid = d >= const(self.min_disp)                # (false for NaN)
            z = torch.where(valid, const(self.fb) / d, const(math.inf))          # tensor / tensor: a correctly rounded fp32 division
            if self.depth == "u16":
                out["depth"] = torch.where(valid, quant(z, self.depth_scale, 65535.0, "u16").to(torch.int32), 0).to(torch.uint16)
            else:
                out["depth"] = z if self.depth == "f32" else z.to(torch.float16)
        if self.uncertainty is not None:
            if u is None:
                raise ValueError("OutputSpec.reference: an uncertainty plane is requested and no uncertainty was given")
            u = u.float().abs()
            out["uncertainties"] = u if self.uncertainty == "f32" else quant(u, 255.0, 255.0, "u8")
        return out


class _EgressCall:
    """One egress launch as ``cascade`` makes it: the spec, the crop (pad_left, pad_top, H0, W0) inside the padded frame (None: the whole
    frame) and the window-local frame range (None: all frames)."""

    def __init__(self, spec: OutputSpec, crop=None, frames=None):
        if not isinstance(spec, OutputSpec):
            raise TypeError(f"output must be an OutputSpec, got {type(spec).__name__}")
        self.spec, self.crop, self.frames = spec, (None if crop is None else tuple(int(x) for x in crop)), (None if frames is None else tuple(int(x) for x in frames))

    def launch(self, eng) -> Dict[str, torch.Tensor]:
        """Allocates the planes on the current stream and enqueues the launch there, behind the engine's last iteration."""
        pad_left, pad_top, h0, w0 = (0, 0, 4 * eng.h, 4 * eng.w) if self.crop is None else self.crop
        f0, f1 = (0, eng.T) if self.frames is None else self.frames
        if not 0 <= f0 < f1 <= eng.T:
            raise ValueError(f"output: frames = {(f0, f1)} is no range inside the window's {eng.T} frames")
        planes = self.spec.empty(f1 - f0, h0, w0, eng.FLOW_OUT.device)
        eng.egress(self.spec.struct(planes), f0, f1 - f0, pad_left, pad_top, h0, w0)
        return planes


class ClipPipeline:
    """Software pipeline over CONSECUTIVE clips / sliding windows (independent units, ppmstereo.py:277-307): the 1/16 and 1/8 scales of
    a clip are latency bound (~70 small launches per iteration, a quarter of a clip's time for 7 % of its FLOPs) and leave most of the
    chip idle, the 1/4 scale is throughput bound.  With the scales on two HIP streams -- ``small`` (1/16, 1/8) and ``large`` (1/4) --
    the small scales of clip k + 1 run under the 1/4 scale of clip k.  Results are the same bits as the unpipelined cascade; what is
    shared between the two stages of consecutive clips (the 1/8 engine's state, read by the 1/4 scale's prologue) is guarded by events.

        pipe = ClipPipeline(device)
        for feats in clips:
            disp, unc = model.cascade(feats, iters, T, test_mode=True, pipeline=pipe)     # enqueues; the result is valid after ...
            ...
        pipe.wait()                                                                        # ... the caller's stream has waited here

    ``cascade`` returns tensors produced on ``large``; ``wait()`` makes the current stream wait for everything enqueued so far (no host
    synchronisation), ``wait(handle)`` for one clip (``handle`` = ``pipe.last``: the completion event of the clip just enqueued)."""

    def __init__(self, device=None, small_priority: int = 0):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = device
        self.small = torch.cuda.Stream(device=device, priority=small_priority)
        self.large = torch.cuda.Stream(device=device)
        self.consumed: Optional[torch.cuda.Event] = None      # the previous clip's 1/4-scale prologue has read the 1/8 engine's state
        self.last: Optional[torch.cuda.Event] = None          # completion of the clip enqueued last
        self.serial = False                                   # True: no overlap between clips (per-launch timing runs of bench.py)
        self.done_events: List[torch.cuda.Event] = []         # (timing: one per clip when ``record_done`` is set)
        self.record_done = False

        self._results: List[torch.Tensor] = []                # tensors handed out by cascade() since the last wait()
        self._health: List[tuple] = []                        # (completion event, diagnostics dict, {scale: device snapshot of the attention counters}) per clip

    def wait(self, handle: Optional[torch.cuda.Event] = None):
        """Orders the current stream behind the clips enqueued so far AND tells the caching allocator that the tensors ``cascade`` returned
        (allocated on ``large``) are now used on the current stream: a caller may launch asynchronous kernels on them and drop them
        without the block being handed to the next clip's 1/4 scale while such a kernel still reads it."""
        ev = self.last if handle is None else handle
        cur = torch.cuda.current_stream(self.device)
        if ev is not None:
            cur.wait_event(ev)
        for t in self._results:
            t.record_stream(cur)
        self._results.clear()
        self._read_health(handle, cur)

    def _read_health(self, handle, cur):
        """cascade(diagnostics=...) left device snapshots of the engines' attention counters for every clip enqueued: those of the clips the
        current stream has now waited for (all, or up to ``handle``'s) are read here -- the host waits for the current stream, which the caller
        of wait() is about to do for the results anyway -- and added to their dicts."""
        n = len(self._health) if handle is None else next((i + 1 for i, item in enumerate(self._health) if item[0] is handle), 0)
        done, self._health = self._health[:n], self._health[n:]
        if not done:
            return
        with torch.cuda.device(self.device), torch.cuda.stream(cur):
            for _, _, snaps in done:
                for s in snaps.values():
                    s.record_stream(cur)
            table = torch.stack([s for _, _, snaps in done for s in snaps.values()])
            cur.synchronize()
            rows = iter(table.tolist())
        for _, diagnostics, snaps in done:
            _add_attn_redo(diagnostics, {tag: dict(zip(("calls", "tiles", "flagged"), next(rows))) for tag in snaps})


class PPMStereoHotPath(nn.Module):
    """The part of PPMStereo that lives on the hot path (ppmstereo.py:82-117 modules, :426-594 loop, :696-804
    cascade), from the encoder / SST outputs on.  Attribute names follow the reference."""

    def __init__(self, max_disp: int = 192, mixed_precision: bool = False, num_frames: int = 5,
                 attention_type: Optional[str] = "self_stereo_temporal_update_time_update_space", use_3d_update_block: bool = True,
                 different_update_blocks: bool = True, use_convex_3d: bool = False, init_flow: bool = False):
        super().__init__()
        if not (use_3d_update_block and different_update_blocks) or init_flow:
            raise NotImplementedError("supported configurations: models/ppm_stereo_model.py:27-33 (use_3d_update_block=True, "
                                      "different_update_blocks=True, init_flow=False) with use_convex_3d False or True (train.py / test.py default)")
        self.hidden_dim = self.context_dim = 128
        self.mixed_precision = mixed_precision      # the engine's precision is fixed: fp32-accurate convs, bf16 attention
        self.use_convex_3d = bool(use_convex_3d)
        self.num_frames = num_frames
        self.att = nn.ModuleList([Attention_qk(num_heads=1, dim_head=128) for _ in range(3)])
        c3 = self.use_convex_3d
        self.update_block08 = SequenceUpdateBlock3D(hidden_dim=128, cor_planes=36, mask_size=4, use_convex_3d=c3)
        self.update_block16 = SequenceUpdateBlock3D(hidden_dim=128, cor_planes=36, mask_size=4, use_convex_3d=c3, attention_type=attention_type)
        self.update_block04 = SequenceUpdateBlock3D(hidden_dim=128, cor_planes=36, mask_size=4, use_convex_3d=c3)

    forward_update_block = forward_update_block

    def convex_upsample(self, flow, mask, rate: int = 4):
        return convex_upsample(flow, mask, rate)

    def convex_upsample_3d(self, flow, mask, rate: int, T: int):
        """PPMStereo.convex_upsample_3d, ppmstereo.py:199-228: flow (b*T,2,H,W), mask (b*T,432,H,W) -> (b*T,2,4H,4W); b = 1."""
        return convex_upsample_3d(flow, mask, rate, T)

    def zero_init(self, fmap: torch.Tensor) -> torch.Tensor:
        """ppmstereo.py:231-236."""
        N, _, H, W = fmap.shape
        return torch.zeros(N, 2, H, W, dtype=torch.float32, device=fmap.device)

    def load_hot_path_weights(self, weights: Dict[str, Dict[str, torch.Tensor]]):
        """weights: {"update_block16": sd, ..., "att.0": sd, ...} (ppmstereo_amd.weights.hot_path_weights)."""
        for tag in ("update_block16", "update_block08", "update_block04"):
            getattr(self, tag).load_state_dict(weights[tag], strict=True)
        for i in range(3):
            self.att[i].load_state_dict(weights[f"att.{i}"], strict=True)
        return self

    @torch.no_grad()
    def cascade(self, feats: Dict[str, torch.Tensor], iters: int, t: int, predictions: Optional[list] = None,
                uncertainties: Optional[list] = None, shard=None, test_mode: bool = False, pipeline: Optional[ClipPipeline] = None,
                diagnostics: Optional[dict] = None, egress: Optional[_EgressCall] = None):
        """The 1/16 -> 1/8 -> 1/4 cascade of PPMStereo.forward (ppmstereo.py:696-804), device resident: the state handed from
        scale to scale (hidden state, motion hidden state) stays in the engines' SP buffers (ppms_sp_resize_blend), only the
        2-channel flow passes through an NCHW resize.  feats: f1_s, f2_s, net_s, inp_s for s in (16, 8, 4) on the GPU
        (with ``shard``: this rank's frames only).  test_mode: only the final prediction is produced (ppmstereo.py:801-804).
        pipeline: a ``ClipPipeline`` -- the small scales and the 1/4 scale are enqueued on its two streams so that consecutive clips
        overlap (same results; see the class).
        diagnostics: a dict -- the fix-up accounting of the memory read-out (ScaleEngine.enable_attn_health) is switched on for this call on
        the three engines, their counters are zeroed at the start, and on return ``diagnostics["attn_redo"]`` holds {"1/16": {"calls",
        "tiles", "flagged"}, "1/8": ..., "1/4": ...}, ADDED to entries already there (one dict over several windows sums them; with
        ``shard``: this rank's clips).  One extra small launch per iteration and one host synchronisation at the end of the call; with a
        ``pipeline`` there is none here: the counters are read in ``ClipPipeline.wait()``.  None (default): nothing is launched or read.
        egress (test_mode, b = 1, no shard): an ``_EgressCall`` -- after the last 1/4-scale iteration ONE ppms_disparity_egress launch on that
        scale's stream replaces the final clone + bilinear pair and writes the requested planes (crop, frame range, formats); the call
        then returns {"disparity", "depth"?, "uncertainties"?}: device tensors (n, 1, H0, W0), and appends nothing to the lists.
        Returns (flow_up (T,1,H,W), uncertainty (T,1,H,W)) = predictions[-1], uncertainties[-1]."""
        if egress is not None:
            if not test_mode:
                raise NotImplementedError("cascade: output planes replace the final prediction only; the per-iteration lists of test_mode=False stay float32")
            if shard is not None:
                raise NotImplementedError("cascade: output planes need the whole window on one GPU; the sharded gather moves float32")
            if feats["f1_16"].shape[0] != t:
                raise NotImplementedError("cascade: output planes are written for one clip per call (b = 1); the batched glue keeps float32 lists")
        if iters < 2:
            raise ValueError(f"cascade: iters={iters}; the 1/16 and 1/8 scales run iters // 2 iterations each (ppmstereo.py:708,744) and need at least one")
        preds = [] if predictions is None else predictions
        uncs = [] if uncertainties is None else uncertainties
        dev = feats["f1_16"].device
        tl = feats["f1_16"].shape[0]                      # frames on this rank (== t without sharding)
        if shard is None and tl != t:
            if tl % t or pipeline is not None:
                raise RuntimeError(f"cascade: {tl} frames do not divide into clips of t = {t} (or a pipeline was given for a batch)")
            if diagnostics is not None:
                raise NotImplementedError("cascade: diagnostics are collected for one clip per call (b = 1)")
            return self._cascade_batched(feats, iters, t, preds, uncs)
        if t == 1:
            warnings.warn("PPMStereo with a single frame produces NaN disparities (reference behaviour, T must be >= 2)")
        lib = L.load()
        with torch.cuda.device(dev):
            caller = torch.cuda.current_stream()
            if pipeline is not None:
                pipeline.small.wait_stream(caller)        # the inputs were produced on the caller's stream
                if pipeline.serial and pipeline.last is not None:
                    pipeline.small.wait_event(pipeline.last)
            prev, fo = None, None
            health = {}                                       # scale -> engine (read below) or device snapshot (read in ClipPipeline.wait)
            for s_, blk, ai, n_it, isc in ((16, self.update_block16, 0, iters // 2, 4), (8, self.update_block08, 1, iters // 2, 2),
                                          (4, self.update_block04, 2, iters, 1)):
                f1, f2 = feats[f"f1_{s_}"], feats[f"f2_{s_}"]
                h, w = f1.shape[2:]
                stream = caller if pipeline is None else (pipeline.large if s_ == 4 else pipeline.small)
                if pipeline is not None:
                    if s_ == 8 and pipeline.consumed is not None:
                        stream.wait_event(pipeline.consumed)      # the previous clip's 1/4 scale still reads this engine's state in its prologue
                    if s_ == 4:
                        stream.wait_stream(pipeline.small)        # this clip's 1/16 and 1/8 scales
                    for k in (f"f1_{s_}", f"f2_{s_}", f"net_{s_}", f"inp_{s_}"):
                        feats[k].record_stream(stream)            # (allocated on the caller's stream: keep the allocator from recycling them early)
                with torch.cuda.stream(stream):
                    eng = blk.engine(tl, h, w, dev, shard)
                    if diagnostics is not None:
                        health_was_on = eng._health_on
                        eng.enable_attn_health(True)
                        eng.reset_attn_health()
                    eng.set_inp(feats[f"inp_{s_}"])
                    eng.set_net(feats[f"net_{s_}"])
                    if prev is None:
                        eng.set_flow(self.zero_init(f1))                                                  # :231-236, :695
                        eng.set_mhs(None)
                    else:
                        ph, pw = prev.h, prev.w
                        eng.set_flow(bilinear(fo, (h, w), True, -(h / fo.shape[2])))                      # :724-725, :760-761 (sign flip kept)
                        eng.parity, eng.have_mhs = 0, True                                                # :726-727, :763-764: mhs x2
                        L.check(lib.ppms_sp_resize_blend(prev.mhs_view(), eng.mhs_view(), tl, ph, pw, 2 * ph, 2 * pw, 0.0, 1.0, L.stream_ptr()))
                        # :729-732, :765-767: net = (net_s + interp(net_2s)) / 2
                        L.check(lib.ppms_sp_resize_blend(prev.net_view(), eng.net_view(), tl, ph, pw, 2 * ph, 2 * pw, 0.5, 0.5, L.stream_ptr()))
                    if pipeline is not None and s_ == 4:
                        pipeline.consumed = torch.cuda.Event()
                        pipeline.consumed.record()                # the 1/8 engine's flow / hidden states have been read: the next clip may overwrite them
                    eng.begin(CorrBlock1D(f1, f2).levels, self.att[ai].packed(dev))
                    last_scale_emit = "none" if egress is not None else "last"       # (the last iteration upsamples its flow either way)
                    fo = _run_iterations(eng, n_it, isc, tl, h, w, preds, uncs, "all" if not test_mode else (last_scale_emit if s_ == 4 else "none"))
                    if egress is not None and s_ == 4:
                        # on this scale's stream and -- with a pipeline -- before ``pipeline.last`` is recorded: the next clip's 1/4 scale
                        # overwrites FLOW_OUT and UNC
                        planes = egress.launch(eng)
                    prev = eng
                    if diagnostics is not None:
                        eng.enable_attn_health(health_was_on)
                        health[f"1/{s_}"] = eng if pipeline is None else eng.attn_health_snapshot()
            if pipeline is not None:
                pipeline.last = torch.cuda.Event(enable_timing=pipeline.record_done)
                pipeline.last.record(pipeline.large)
                if diagnostics is not None:
                    pipeline._health.append((pipeline.last, diagnostics, health))
                    del pipeline._health[:-16]                     # (as _results below: a caller that never waits)
                if pipeline.record_done:
                    pipeline.done_events.append(pipeline.last)
                pipeline._results += [preds[-1], uncs[-1]] if egress is None else list(planes.values())      # (ClipPipeline.wait records the consuming stream on them)
                del pipeline._results[:-16]                        # a caller that never waits (bench.py) must not accumulate references
            elif diagnostics is not None:
                _add_attn_redo(diagnostics, {tag: eng.attn_health() for tag, eng in health.items()})
            return planes if egress is not None else (preds[-1], uncs[-1])


def _cascade_batched(self, feats, iters: int, t: int, preds: list, uncs: list):
    """cascade for b > 1 clips (frame index = bi * t + ti, ppmstereo.py:443-449): the reference's glue between the three
    forward_update_block calls (:696-791) on NCHW tensors -- every iteration's prediction is produced, as test_mode=False does.  The batch
    elements meet in one scalar per clip index only (the mean of the picked scores, :533), which forward_update_block reproduces; b = 1 --
    the reference's inference entry -- takes the device-resident path above instead."""
    f16 = feats["f1_16"]
    fo, net16, mhs16 = self.forward_update_block(None, self.update_block16, CorrBlock1D(f16, feats["f2_16"]), self.zero_init(f16), feats["net_16"],
                                                 feats["inp_16"], None, self.att[0], preds, uncs, iters // 2, 4, t)                 # :707-722
    nets, mhs = {16: net16}, {16: mhs16}
    for s_, blk, ai, n_it, isc in ((8, self.update_block08, 1, iters // 2, 2), (4, self.update_block04, 2, iters, 1)):
        f1, f2 = feats[f"f1_{s_}"], feats[f"f2_{s_}"]
        h, w = f1.shape[2:]
        flow = bilinear(fo, (h, w), True, -(h / fo.shape[2]))                                                                       # :724-725, :760-761
        m_up = bilinear(mhs[2 * s_], (h, w), True)                                                                                   # :726-727, :763-764
        net = (feats[f"net_{s_}"] + bilinear(nets[2 * s_], (h, w), True)) / 2.0                                                     # :729-732, :765-767
        fo, nets[s_], mhs[s_] = self.forward_update_block(None, blk, CorrBlock1D(f1, f2), flow, net, feats[f"inp_{s_}"], m_up, self.att[ai],
                                                          preds, uncs, n_it, isc, t)                                                # :743-758, :776-791
    return preds[-1], uncs[-1]


PPMStereoHotPath._cascade_batched = _cascade_batched


def position_encoding_sine(d_model: int, h: int, w: int) -> torch.Tensor:
    """PositionEncodingSine (temp_bug_fix=True), models/core/attention.py:23-64 -> (d_model, h, w); host table, same torch
    op sequence as the reference (built once per geometry)."""
    pe = torch.zeros((d_model, h, w))
    y_position = torch.ones((h, w)).cumsum(0).float().unsqueeze(0)
    x_position = torch.ones((h, w)).cumsum(1).float().unsqueeze(0)
    div_term = torch.exp(torch.arange(0, d_model // 2, 2).float() * (-math.log(10000.0) / (d_model // 2)))[:, None, None]
    pe[0::4, :, :] = torch.sin(x_position * div_term)
    pe[1::4, :, :] = torch.cos(x_position * div_term)
    pe[2::4, :, :] = torch.sin(y_position * div_term)
    pe[3::4, :, :] = torch.cos(y_position * div_term)
    return pe


class InputPadder:
    """Replicate-pads the last two dimensions up to multiples of ``divis_by`` and crops results back (the reference's helper,
    models/core/utils/utils.py:19-44).  "sintel" mode centres the image (the extra row / column of an odd pad goes to the bottom /
    right); any other mode pads the height at the bottom only."""

    def __init__(self, dims, mode: str = "sintel", divis_by: int = 8):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        extra_h, extra_w = -self.ht % divis_by, -self.wd % divis_by
        left, top = extra_w // 2, (extra_h // 2 if mode == "sintel" else 0)
        self._pad = [left, extra_w - left, top, extra_h - top]          # F.pad order: left, right, top, bottom

    def geometry(self):
        """(pad_left, pad_top, H, W): the columns / rows ``pad`` adds in front and the padded size (what ppms_video_ingest_u8 takes)."""
        left, right, top, bottom = self._pad
        return left, top, top + self.ht + bottom, left + self.wd + right

    def pad(self, *inputs):
        for x in inputs:
            if x.ndim != 4:
                raise ValueError(f"InputPadder.pad: 4-D tensors expected, got {tuple(x.shape)}")
        if not any(self._pad):
            return list(inputs)                                           # (already a multiple: nothing to copy)
        return [torch.nn.functional.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        if x.ndim != 4:
            raise ValueError(f"InputPadder.unpad: 4-D tensor expected, got {tuple(x.shape)}")
        left, right, top, bottom = self._pad
        return x[..., top:x.shape[-2] - bottom, left:x.shape[-1] - right]


_BYTE_LUT: Dict[int, torch.Tensor] = {}


def byte_lut(device) -> torch.Tensor:
    """fp32 [256] on `device`: the normalised value of every byte, from the expression ``forward`` applies to float images ON THE SAME
    DEVICE -- torch's division by a Python scalar need not round like a division written elsewhere, so the table is what makes the uint8
    path the float path's bits.  Built once per device (the host waits for it once)."""
    device = torch.device(device)
    idx = torch.cuda.current_device() if device.index is None else device.index
    if idx not in _BYTE_LUT:
        dev = torch.device("cuda", idx)
        _BYTE_LUT[idx] = (2 * (torch.arange(256, dtype=torch.float32, device=dev) / 255.0) - 1.0).contiguous()
        torch.cuda.current_stream(dev).synchronize()             # later calls may read it from any stream
    return _BYTE_LUT[idx]


class _ByteFrames:
    """uint8 frames of both views on the device as ppms_video_ingest_u8 reads them: ``left`` / ``right`` start at frame 0 of a view, frame
    n of a view lies ``frame_stride`` bytes further; (H0, W0) frames go to the padded size with ``pad_left`` / ``pad_top`` in front."""

    def __init__(self, left: torch.Tensor, right: torch.Tensor, frame_stride: int, n: int, h0: int, w0: int, pad_left: int = 0, pad_top: int = 0,
                 rectify: Optional["StereoRectifier"] = None):
        self.left, self.right, self.frame_stride, self.n = left, right, int(frame_stride), int(n)
        self.h0, self.w0, self.pad_left, self.pad_top = int(h0), int(w0), int(pad_left), int(pad_top)
        self.rectify = rectify                                  # on the frames' device: they are raw frames of its source size, (h0, w0) its rectified size

    def ingest(self, dst_fnet: L.SP, dst_cnet: L.SP, h: int, w: int) -> None:
        """One launch on the current stream: both encoders' first-layer operands of the n frames padded to h x w."""
        if self.rectify is not None:
            lmap, rmap = self.rectify.left.view_struct(), self.rectify.right.view_struct()       # host structs: read before the call returns
            L.check(L.load().ppms_video_ingest_u8_remap(self.left.data_ptr(), self.right.data_ptr(), self.frame_stride, lmap, rmap, self.n, self.h0, self.w0,
                                                        self.pad_left, self.pad_top, h, w, byte_lut(self.left.device).data_ptr(), dst_fnet, dst_cnet,
                                                        L.stream_ptr()))
            return
        L.check(L.load().ppms_video_ingest_u8(self.left.data_ptr(), self.right.data_ptr(), self.frame_stride, self.n, self.h0, self.w0, self.pad_left,
                                              self.pad_top, h, w, byte_lut(self.left.device).data_ptr(), dst_fnet, dst_cnet, L.stream_ptr()))

    def held(self):
        """The tensors the launch reads (for record_stream)."""
        if self.rectify is not None:
            return (self.left, self.right) + self.rectify.tensors()
        return self.left, self.right


_YUV_STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}       # (Kr, Kb)


def yuv_matrix(standard: str = "bt709", full_range: bool = False, shift: int = 14) -> L.YUVMatrix:
    """The fixed-point YCbCr -> RGB conversion ppms_video_ingest_yuv420 applies (include/ppms.h), as its ``ppms_yuv_matrix``: Python
    ``round()`` of the double-precision coefficients times 2^shift.  Limited range: Y in [16, 235], chroma in [16, 240]."""
    if standard not in _YUV_STANDARDS:
        raise ValueError(f"yuv_matrix: standard {standard!r}; one of {sorted(_YUV_STANDARDS)}")
    if not 8 <= shift <= 20:
        raise ValueError(f"yuv_matrix: shift = {shift} must lie in [8, 20]")
    kr, kb = _YUV_STANDARDS[standard]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    one = float(1 << shift)
    return L.YUVMatrix(y_off=0 if full_range else 16, cy=round(sy * one), crv=round(sc * 2.0 * (1.0 - kr) * one),
                       cgu=round(sc * 2.0 * kb * (1.0 - kb) / kg * one), cgv=round(sc * 2.0 * kr * (1.0 - kr) / kg * one),
                       cbu=round(sc * 2.0 * (1.0 - kb) * one), shift=shift, reserved=0)


class YUVFrames:
    """One view's N decoded 8-bit YUV 4:2:0 frames, as a decoder leaves them: ``y`` uint8 (N, H0, W0), ``u`` / ``v`` uint8
    (N, ceil(H0 / 2), ceil(W0 / 2)).  Each may be a strided VIEW of a decoder surface -- a pitched plane, the two halves of an interleaved
    UV plane (``nv12``), one half of a frame that packs both views (``split_side_by_side`` / ``split_top_bottom``): the class reads
    ``data_ptr()`` and ``stride()`` and never copies.  ``y`` needs last-dimension stride 1; ``u`` and ``v`` equal strides with
    last-dimension stride 1 (planar: I420 / yuv420p) or 2 (interleaved: NV12); anything else raises ValueError.  Luma pixel (y, x) takes
    chroma sample (y >> 1, x >> 1); ``standard`` ("bt709" / "bt601") and ``full_range`` choose ``yuv_matrix``; ``to_rgb_u8`` is the
    definition of the RGB bytes.  Not covered: 10-bit surfaces (P010), 4:2:2 and 4:4:4, interpolated chroma siting, b > 1."""

    def __init__(self, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, standard: str = "bt709", full_range: bool = False):
        for name, t in (("y", y), ("u", u), ("v", v)):
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3:
                raise ValueError(f"YUVFrames: {name} must be a uint8 tensor (N, rows, columns)")
        n, h0, w0 = y.shape
        hc, wc = (h0 + 1) // 2, (w0 + 1) // 2
        if n < 1 or h0 < 1 or w0 < 1:
            raise ValueError(f"YUVFrames: empty y plane {tuple(y.shape)}")
        if tuple(u.shape) != (n, hc, wc) or tuple(v.shape) != (n, hc, wc):
            raise ValueError(f"YUVFrames: y {tuple(y.shape)} needs u and v of {(n, hc, wc)}, got {tuple(u.shape)} and {tuple(v.shape)}")
        if u.device != y.device or v.device != y.device:
            raise ValueError("YUVFrames: y, u and v must be on one device")
        if w0 > 1 and y.stride(2) != 1:
            raise ValueError(f"YUVFrames: y has last-dimension stride {y.stride(2)}; luma samples must be adjacent bytes")
        step = u.stride(2) if wc > 1 else 1                                # (a one-column chroma plane never takes a step)
        if u.stride() != v.stride():
            raise ValueError(f"YUVFrames: u and v must have equal strides, got {u.stride()} and {v.stride()}")
        if step not in (1, 2):
            raise ValueError(f"YUVFrames: chroma last-dimension stride {step}; 1 (planar) or 2 (interleaved) expected")
        # a size-1 dimension's stride is arbitrary: the smallest the kernel accepts stands in for it
        self.pitch_y = y.stride(1) if h0 > 1 else w0
        self.pitch_c = u.stride(1) if hc > 1 else step * (wc - 1) + 1
        self.step_c = step
        self.frame_stride_y = y.stride(0) if n > 1 else (h0 - 1) * self.pitch_y + w0
        self.frame_stride_c = u.stride(0) if n > 1 else (hc - 1) * self.pitch_c + step * (wc - 1) + 1
        if (self.pitch_y < w0 or self.pitch_c < step * (wc - 1) + 1 or self.frame_stride_y < (h0 - 1) * self.pitch_y + w0
                or self.frame_stride_c < (hc - 1) * self.pitch_c + step * (wc - 1) + 1):
            raise ValueError(f"YUVFrames: rows or frames overlap (y strides {y.stride()}, chroma strides {u.stride()})")
        yuv_matrix(standard)                                               # (refuses an unknown standard here)
        self.y, self.u, self.v, self.standard, self.full_range = y, u, v, standard, bool(full_range)
        self.n, self.height, self.width = n, h0, w0

    @classmethod
    def nv12(cls, y: torch.Tensor, uv: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """NV12: ``uv`` uint8 (N, ceil(H0 / 2), ceil(W0 / 2), 2), U first -- a hardware decoder's surface."""
        if not torch.is_tensor(uv) or uv.dim() != 4 or uv.shape[-1] != 2:
            raise ValueError("YUVFrames.nv12: uv must be (N, rows, columns, 2)")
        return cls(y, uv[..., 0], uv[..., 1], standard, full_range)

    @classmethod
    def i420(cls, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, standard: str = "bt709", full_range: bool = False) -> "YUVFrames":
        """I420 / yuv420p: three planes -- a software decoder's frame."""
        return cls(y, u, v, standard, full_range)

    def __len__(self) -> int:
        return self.n

    @property
    def device(self) -> torch.device:
        return self.y.device

    def _like(self, y, u, v) -> "YUVFrames":
        return YUVFrames(y, u, v, self.standard, self.full_range)

    def __getitem__(self, frames: slice) -> "YUVFrames":
        if not isinstance(frames, slice):
            raise TypeError("YUVFrames: index with a slice of frames")
        return self._like(self.y[frames], self.u[frames], self.v[frames])

    def split_side_by_side(self):
        """(left, right): the two halves of frames that pack both views side by side; views, no copy.  The packed width must be even --
        and each half's too, or the right half's chroma would start between two samples."""
        w = self.width
        if w % 2 or (w // 2) % 2:
            raise ValueError(f"YUVFrames.split_side_by_side: a packed width of {w} does not split into two views with whole chroma samples")
        h, q = w // 2, w // 4
        return (self._like(self.y[:, :, :h], self.u[:, :, :q], self.v[:, :, :q]), self._like(self.y[:, :, h:], self.u[:, :, q:], self.v[:, :, q:]))

    def split_top_bottom(self):
        """(left, right) = (top, bottom) halves of frames that pack both views one above the other; views, no copy (even halves, as above)."""
        ht = self.height
        if ht % 2 or (ht // 2) % 2:
            raise ValueError(f"YUVFrames.split_top_bottom: a packed height of {ht} does not split into two views with whole chroma rows")
        h, q = ht // 2, ht // 4
        return (self._like(self.y[:, :h], self.u[:, :q], self.v[:, :q]), self._like(self.y[:, h:], self.u[:, q:], self.v[:, q:]))

    def to(self, device) -> "YUVFrames":
        """These frames on ``device``: the planes' own bytes are copied (1.5 per pixel; an interleaved UV plane as one block) into dense
        planes; frames already there are returned as they are."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device == device:
            return self
        y = self.y.to(device)
        if self.step_c == 2 and self.v.data_ptr() == self.u.data_ptr() + 1:
            uv = torch.as_strided(self.u, (*self.u.shape, 2), (*self.u.stride(), 1)).to(device)
            return self._like(y, uv[..., 0], uv[..., 1])
        return self._like(y, self.u.to(device), self.v.to(device))

    def matrix(self) -> L.YUVMatrix:
        return yuv_matrix(self.standard, self.full_range)

    def view_struct(self) -> L.YUVView:
        """The ``ppms_yuv_view`` of these frames."""
        return L.YUVView(self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), self.frame_stride_y, self.frame_stride_c, self.pitch_y, self.pitch_c,
                         self.step_c, 0)

    def to_rgb_u8(self) -> torch.Tensor:
        """uint8 (N, 3, H0, W0) on the same device: the conversion of include/ppms.h in torch integer ops -- what the feature means by the
        RGB bytes of these frames (the kernel's operands are ppms_video_ingest_u8's on them), and the path where the kernel cannot be used."""
        m = self.matrix()
        rows = torch.arange(self.height, device=self.device) >> 1
        cols = torch.arange(self.width, device=self.device) >> 1
        d = self.y.to(torch.int32) - m.y_off
        e, f = (c.to(torch.int32)[:, rows][:, :, cols] - 128 for c in (self.u, self.v))
        r = 1 << (m.shift - 1)
        rgb = torch.stack([m.cy * d + m.crv * f + r, m.cy * d - m.cgu * e - m.cgv * f + r, m.cy * d + m.cbu * e + r], dim=1)
        return (rgb >> m.shift).clamp_(0, 255).to(torch.uint8)


class YUVStereoVideo:
    """Both views of a decoded 4:2:0 video -- what ``batch_dict["stereo_video"]`` of ``forward_batch_test`` may be instead of a tensor:
    two ``YUVFrames`` of one size, frame count, device and colour description.  ``len()``, slicing by frame range, ``to(device)``."""

    def __init__(self, left: YUVFrames, right: YUVFrames):
        if not isinstance(left, YUVFrames) or not isinstance(right, YUVFrames):
            raise TypeError("YUVStereoVideo: two YUVFrames expected")
        if (left.n, left.height, left.width) != (right.n, right.height, right.width):
            raise ValueError(f"YUVStereoVideo: the views differ: {(left.n, left.height, left.width)} and {(right.n, right.height, right.width)}")
        if (left.standard, left.full_range) != (right.standard, right.full_range) or left.device != right.device:
            raise ValueError("YUVStereoVideo: both views need one standard, one range and one device")
        self.left, self.right = left, right
        self.height, self.width = left.height, left.width

    def __len__(self) -> int:
        return self.left.n

    def __getitem__(self, frames: slice) -> "YUVStereoVideo":
        return YUVStereoVideo(self.left[frames], self.right[frames])

    def to(self, device) -> "YUVStereoVideo":
        """The selected frames' planes on ``device`` (1.5 bytes per pixel and view)."""
        return YUVStereoVideo(self.left.to(device), self.right.to(device))


class _YUVPlanes:
    """``_ByteFrames`` for a YUVStereoVideo on the device: ppms_video_ingest_yuv420 converts, pads and lays out both views in one launch."""

    def __init__(self, video: YUVStereoVideo, pad_left: int = 0, pad_top: int = 0, rectify: Optional["StereoRectifier"] = None):
        self.video, self.pad_left, self.pad_top = video, int(pad_left), int(pad_top)
        self.rectify = rectify                                  # on the video's device: the video holds raw frames of its source size

    def ingest(self, dst_fnet: L.SP, dst_cnet: L.SP, h: int, w: int) -> None:
        v = self.video
        left, right, m = v.left.view_struct(), v.right.view_struct(), v.left.matrix()      # host structs: read before the call returns
        if self.rectify is not None:
            r = self.rectify
            L.check(L.load().ppms_video_ingest_yuv420_remap(left, right, m, r.left.view_struct(), r.right.view_struct(), len(v), r.height, r.width,
                                                            self.pad_left, self.pad_top, h, w, byte_lut(v.left.device).data_ptr(), dst_fnet, dst_cnet,
                                                            L.stream_ptr()))
            return
        L.check(L.load().ppms_video_ingest_yuv420(left, right, m, len(v), v.height, v.width, self.pad_left, self.pad_top, h, w,
                                                  byte_lut(v.left.device).data_ptr(), dst_fnet, dst_cnet, L.stream_ptr()))

    def held(self):
        v = self.video
        planes = (v.left.y, v.left.u, v.left.v, v.right.y, v.right.u, v.right.v)
        return planes if self.rectify is None else planes + self.rectify.tensors()


_BORDERS = {"replicate": L.BORDER_REPLICATE, "constant": L.BORDER_CONSTANT}


class RectifyMap:
    """One view's undistort + rectify (+ resize) map in fixed point, as ppms_video_ingest_u8_remap / _yuv420_remap read it (the arithmetic:
    include/ppms.h): for every pixel of the RECTIFIED frame H0 x W0, ``xy`` int16 (H0, W0, 2) holds the integer source coordinate (x0, y0), x
    first, and ``frac`` int16 or uint16 (H0, W0) its fraction in 1/32 pixel, fx | fy << 5 -- the layout OpenCV documents for
    ``convertMaps(..., CV_16SC2)`` (not compared with OpenCV).  ``source_size`` = (Hs, Ws) of the raw frames; ``border`` "replicate" or
    "constant" (a tap outside the frame is ``fill``, one byte for R, G and B).  Both tensors may be row-pitched views with ONE pitch
    (``xy.stride(0) == 2 * frac.stride(0)``): the class reads ``data_ptr()`` and ``stride()`` and never copies.  ``apply_u8`` is the definition
    of the remap.  Not covered: computing maps from calibration data, interpolation other than bilinear."""

    def __init__(self, xy: torch.Tensor, frac: torch.Tensor, source_size, border: str = "replicate", fill: int = 0, _checked: bool = False):
        if not torch.is_tensor(xy) or xy.dtype != torch.int16 or xy.dim() != 3 or xy.shape[2] != 2:
            raise ValueError("RectifyMap: xy must be an int16 tensor (H0, W0, 2)")
        if not torch.is_tensor(frac) or frac.dtype not in (torch.int16, torch.uint16) or frac.dim() != 2:
            raise ValueError("RectifyMap: frac must be an int16 or uint16 tensor (H0, W0)")
        h0, w0 = frac.shape
        if h0 < 1 or w0 < 1 or tuple(xy.shape[:2]) != (h0, w0):
            raise ValueError(f"RectifyMap: xy {tuple(xy.shape)} and frac {tuple(frac.shape)} must cover one non-empty frame")
        if xy.device != frac.device:
            raise ValueError("RectifyMap: xy and frac must be on one device")
        frac = frac.view(torch.int16)                               # the same 16 bits
        if xy.stride(2) != 1 or (w0 > 1 and (xy.stride(1) != 2 or frac.stride(1) != 1)):
            raise ValueError(f"RectifyMap: the last dimensions must be contiguous (xy strides {xy.stride()}, frac strides {frac.stride()})")
        # a size-1 dimension's stride is arbitrary: the smallest the kernel accepts stands in for it
        pitch = frac.stride(0) if h0 > 1 else w0
        if pitch < w0 or (h0 > 1 and xy.stride(0) != 2 * pitch):
            raise ValueError(f"RectifyMap: xy and frac need one row pitch >= W0 (xy strides {xy.stride()}, frac strides {frac.stride()})")
        if xy.data_ptr() % 4 or frac.data_ptr() % 2:
            raise ValueError("RectifyMap: xy must start at a multiple of 4 bytes, frac of 2")
        try:
            hs, ws = (int(v) for v in source_size)
        except (TypeError, ValueError):
            raise ValueError(f"RectifyMap: source_size = {source_size!r} must be (Hs, Ws)") from None
        if not (1 <= hs <= 32768 and 1 <= ws <= 32768):
            raise ValueError(f"RectifyMap: source_size = ({hs}, {ws}) must lie in 1..32768")
        if border not in _BORDERS:
            raise ValueError(f"RectifyMap: border {border!r}; one of {sorted(_BORDERS)}")
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"RectifyMap: fill = {fill} must be a byte")
        if not _checked and bool(((frac < 0) | (frac > 1023)).any()):      # once: copies made by ``to`` hold the same values
            raise ValueError("RectifyMap: frac holds values above 1023 (fx | fy << 5 with fx, fy in 0..31)")
        self.xy, self.frac, self.pitch = xy, frac, int(pitch)
        self.height, self.width, self.source_height, self.source_width = int(h0), int(w0), hs, ws
        self.border, self.fill = border, int(fill)
        self._on: Dict[torch.device, "RectifyMap"] = {xy.device: self}

    @classmethod
    def from_float(cls, map_x: torch.Tensor, map_y: torch.Tensor, source_size, border: str = "replicate", fill: int = 0) -> "RectifyMap":
        """From float source coordinates (H0, W0) per rectified pixel (what ``initUndistortRectifyMap`` gives as CV_32FC1): per coordinate
        q = round_half_even(v * 32), saturated so that q >> 5 stays an int16; then x0 = q >> 5, fx = q & 31 (floor and remainder)."""
        if not (torch.is_tensor(map_x) and torch.is_tensor(map_y) and map_x.is_floating_point() and map_y.is_floating_point()
                and map_x.dim() == 2 and map_x.shape == map_y.shape):
            raise ValueError("RectifyMap.from_float: map_x and map_y must be floating-point tensors of one shape (H0, W0)")
        if bool(torch.isnan(map_x).any()) or bool(torch.isnan(map_y).any()):
            raise ValueError("RectifyMap.from_float: a coordinate is NaN")
        qx, qy = (torch.round(m.double() * 32.0).clamp(-32768 * 32, 32767 * 32 + 31).to(torch.int64) for m in (map_x, map_y))
        xy = torch.stack([qx >> 5, qy >> 5], dim=-1).to(torch.int16)
        frac = ((qx & 31) | ((qy & 31) << 5)).to(torch.int16)
        return cls(xy, frac, source_size, border, fill, _checked=True)

    @classmethod
    def identity(cls, h: int, w: int, device=None) -> "RectifyMap":
        """The map that copies an h x w frame."""
        ys, xs = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
        return cls(torch.stack([xs, ys], dim=-1).to(torch.int16), torch.zeros((h, w), dtype=torch.int16, device=device), (h, w), _checked=True)

    @property
    def device(self) -> torch.device:
        return self.xy.device

    def to(self, device) -> "RectifyMap":
        """This map on ``device`` (6 bytes per rectified pixel, dense); made once per device and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            there = RectifyMap(self.xy.to(device).contiguous(), self.frac.to(device).contiguous(), (self.source_height, self.source_width), self.border,
                               self.fill, _checked=True)
            there._on = self._on
            self._on[device] = there
        return self._on[device]

    def view_struct(self) -> L.RemapView:
        """The ``ppms_remap_view`` of this map."""
        return L.RemapView(self.xy.data_ptr(), self.frac.data_ptr(), self.pitch, self.source_height, self.source_width, _BORDERS[self.border], self.fill, 0)

    def apply_u8(self, rgb: torch.Tensor) -> torch.Tensor:
        """uint8 (N, 3, Hs, Ws) -> uint8 (N, 3, H0, W0) on ``rgb``'s device: the remap of include/ppms.h in torch integer ops -- what the feature
        means by the rectified bytes (the kernels' operands are ppms_video_ingest_u8's on them), and the path where the kernels cannot be used."""
        hs, ws = self.source_height, self.source_width
        if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or tuple(rgb.shape[1:]) != (3, hs, ws):
            raise ValueError(f"RectifyMap.apply_u8: uint8 frames (N, 3, {hs}, {ws}) expected, got "
                             f"{tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__}")
        m = self.to(rgb.device)
        x0, y0 = m.xy[..., 0].to(torch.int64), m.xy[..., 1].to(torch.int64)
        f = m.frac.to(torch.int32)
        fx, fy = f & 31, (f >> 5) & 31
        acc = torch.full((rgb.shape[0], 3, self.height, self.width), 512, dtype=torch.int32, device=rgb.device)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                cy, cx = yy.clamp(0, hs - 1), xx.clamp(0, ws - 1)
                p = rgb[:, :, cy, cx].to(torch.int32)             # clamped addresses in both modes
                if self.border == "constant":
                    p = torch.where((cy != yy) | (cx != xx), torch.full_like(p, self.fill), p)
                acc += ((fx if dx else 32 - fx) * (fy if dy else 32 - fy)) * p
        return (acc >> 10).to(torch.uint8)


class StereoRectifier:
    """The two views' ``RectifyMap``s of one rig -- what ``rectify=`` of ``PPMStereo.forward`` / ``forward_batch_test`` takes: one rectified size
    (``height`` x ``width``), one source size (``source_height`` x ``source_width``), one device.  ``to(device)`` is kept per device."""

    def __init__(self, left: RectifyMap, right: RectifyMap):
        if not isinstance(left, RectifyMap) or not isinstance(right, RectifyMap):
            raise TypeError("StereoRectifier: two RectifyMaps expected")
        if (left.height, left.width) != (right.height, right.width):
            raise ValueError(f"StereoRectifier: the rectified sizes differ: {(left.height, left.width)} and {(right.height, right.width)}")
        if (left.source_height, left.source_width) != (right.source_height, right.source_width):
            raise ValueError(f"StereoRectifier: the source sizes differ: {(left.source_height, left.source_width)} and "
                             f"{(right.source_height, right.source_width)}")
        if left.device != right.device:
            raise ValueError("StereoRectifier: both maps must be on one device")
        self.left, self.right = left, right
        self.height, self.width = left.height, left.width
        self.source_height, self.source_width = left.source_height, left.source_width

    @property
    def device(self) -> torch.device:
        return self.left.device

    def to(self, device) -> "StereoRectifier":
        left, right = self.left.to(device), self.right.to(device)
        return self if left is self.left and right is self.right else StereoRectifier(left, right)

    def tensors(self):
        """The four map tensors (for record_stream)."""
        return self.left.xy, self.left.frac, self.right.xy, self.right.frac

    def apply_u8(self, left: torch.Tensor, right: torch.Tensor):
        return self.left.apply_u8(left), self.right.apply_u8(right)

    def check_source(self, who: str, h: int, w: int) -> None:
        if (int(h), int(w)) != (self.source_height, self.source_width):
            raise ValueError(f"{who}: the frames are {int(h)} x {int(w)}, the rectification maps were made for {self.source_height} x {self.source_width}")


class PPMStereo(PPMStereoHotPath):
    """``models/core/ppmstereo.py:PPMStereo`` from the encoder outputs on: same constructor arguments, ``forward`` (:601-804)
    and ``forward_batch_test`` (:238-320).  The encoders are outside the hot path: ``fnet``
    and ``cnet`` default to this package's HIP ``BasicEncoder`` / ``Feature("tiny", 256)`` (``ppmstereo_amd/encoder.py``, ``cnet.py``:
    rows f3, f5; ``False`` leaves one unset), or take any callable with the same contract:
    ``fnet([im1, im2]) -> (fmap1, fmap2)`` (BT,256,H/4,W/4), ``cnet(im1) -> (c4, c8, c16)`` with 256 channels;
    ``sst`` stands for ``forward_sst_block`` (:322-395): "auto" (default) follows the reference's ctor (:139-171) -- the HIP
    ``SSTBlock`` (``ppmstereo_amd/sst.py``, row f4) when ``attention_type`` names "self_stereo" / "temporal", its parameters
    registered under the reference's names (``time_embed``, ``time_attn_blocks``, ``self_attn_blocks``, ``cross_attn_blocks``);
    ``None`` = the ``attention_type=None`` behaviour (positional encoding only); or any callable ``(f1_16, f2_16, T)``.
    Everything between the images (minus cnet) and the returned disparity runs on the gfx950 kernels."""

    # what models/ppm_stereo_model.py:27-33 passes: the configuration of the released model, and the one this implementation serves
    WRAPPER_CONFIG = dict(mixed_precision=True, num_frames=5, attention_type="self_stereo_temporal_update_time_update_space",
                          use_3d_update_block=True, different_update_blocks=True)

    @classmethod
    def shipped(cls, **overrides):
        """PPMStereo(**WRAPPER_CONFIG, **overrides): the model as the reference's wrapper builds it (models/ppm_stereo_model.py:27-33)."""
        return cls(**{**cls.WRAPPER_CONFIG, **overrides})

    def __init__(self, max_disp: int = 192, mixed_precision: bool = False, num_frames: int = 5, attention_type: Optional[str] = None,
                 use_3d_update_block: bool = False, different_update_blocks: bool = False, use_convex_3d: bool = False, init_flow: bool = False,
                 *, fnet=None, cnet=None, sst="auto"):
        """Parameter names, order AND defaults of the reference's constructor (ppmstereo.py:45-55).  The reference's defaults select the 2-D
        update block (use_3d_update_block=False), which this implementation does not serve (and the reference's own forward cannot drive,
        SURVEY.md hazard 7): a default-constructed PPMStereo() therefore raises NotImplementedError naming the supported configuration
        instead of silently building another module tree -- pass the wrapper's arguments, or use ``PPMStereo.shipped()``."""
        if not (use_3d_update_block and different_update_blocks):
            raise NotImplementedError("PPMStereo: the gfx950 implementation serves the released configuration, models/ppm_stereo_model.py:27-33 -- "
                                      "use_3d_update_block=True, different_update_blocks=True (PPMStereo.shipped() / PPMStereo.WRAPPER_CONFIG); the "
                                      "2-D update block selected by the reference's constructor defaults is outside the hot path")
        super().__init__(max_disp, mixed_precision, num_frames, attention_type, use_3d_update_block, different_update_blocks, use_convex_3d, init_flow)
        at = attention_type
        if isinstance(sst, str) and sst == "auto":
            sst = None
            if at is not None and ("self_stereo" in at or "temporal" in at):
                if not ("self_stereo" in at and "temporal" in at):
                    raise NotImplementedError("SST block: attention types with both 'self_stereo' and 'temporal' (the shipped model) or neither")
                from .sst import SSTBlock
                blk = SSTBlock(dim=256, num_frames=self.num_frames)
                self.time_embed = blk.time_embed                       # same objects, registered under the reference's names
                self.time_attn_blocks, self.self_attn_blocks, self.cross_attn_blocks = blk.time_attn_blocks, blk.self_attn_blocks, blk.cross_attn_blocks
                object.__setattr__(self, "_sst_impl", blk)           # (not a second registration of the same parameters)
                sst = blk
        if fnet is None:                                       # the reference builds it in its ctor (ppmstereo.py:64)
            from .encoder import BasicEncoder
            fnet = BasicEncoder(output_dim=256, norm_fn="instance")
        if cnet is None:                                       # (ppmstereo.py:69; no checkpoint is read here: load_state_dict supplies it)
            from .cnet import Feature
            cnet = Feature(model_name="tiny", output_dim=256)
        self.fnet, self.cnet = (None if fnet is False else fnet), (None if cnet is False else cnet)
        object.__setattr__(self, "sst", sst)
        # state_dict in the reference's registration order (ppmstereo.py:64-171): fnet, cnet, att, the update blocks, the SST modules
        ref_order = ["fnet", "cnet", "att", "update_block08", "update_block16", "update_block04", "time_attn_blocks", "self_attn_blocks", "cross_attn_blocks"]
        mods = self._modules
        for k in [k for k in ref_order if k in mods] + [k for k in list(mods) if k not in ref_order]:
            mods[k] = mods.pop(k)                              # (re-insertion moves the key to the end)
        self.dim = 256
        self._pe_cache: Dict[tuple, torch.Tensor] = {}
        self.parallel_encoders = True                          # cnet on a side stream beside fnet (forward)
        self._enc_streams: Dict[int, torch.cuda.Stream] = {}

    def _encoder_stream(self, device) -> torch.cuda.Stream:
        idx = torch.device(device).index or 0
        if idx not in self._enc_streams:
            self._enc_streams[idx] = torch.cuda.Stream(device=device)
        return self._enc_streams[idx]

    def load_state_dict(self, sd, strict: bool = True, **kw):
        r = super().load_state_dict(sd, strict=strict, **kw)
        for m in (self.fnet, self.cnet, getattr(self, "_sst_impl", None)):       # packed weight copies are cached per module
            if hasattr(m, "invalidate"):
                m.invalidate()
        return r

    # ------------------------------------------------------------------ pre-loop glue (ppmstereo.py:620-682)
    def _pe(self, h: int, w: int, device) -> torch.Tensor:
        key = (h, w, str(device))
        if key not in self._pe_cache:
            self._pe_cache[key] = position_encoding_sine(self.dim, h, w).to(device).contiguous()
        return self._pe_cache[key]

    def pre_loop(self, fmap1: torch.Tensor, fmap2: torch.Tensor, c4: torch.Tensor, c8: torch.Tensor, c16: torch.Tensor, t: int, ctx_ready=None):
        """fmap (BT,256,h,w) at 1/4, context features at 1/4, 1/8, 1/16 -> the dict ``cascade`` consumes.
        ctx_ready (optional callable): called once, right before the context features are first read -- ``forward`` passes the wait for the
        stream cnet runs on, so that the pooling and the SST block (which need fnet's output only) do not wait for cnet."""
        L.require_gpu(fmap1, fmap2, c4, c8, c16)
        lib, st = L.load(), L.stream_ptr
        N, C, h, w = fmap1.shape
        if C != 256 or h % 4 or w % 4:
            raise RuntimeError("pre_loop: 256-channel 1/4-resolution features with h, w multiples of 4 expected")
        dev = fmap1.device
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        fm = [fmap1.contiguous().float(), fmap2.contiguous().float()]
        feats: Dict[str, torch.Tensor] = {"f1_4": fm[0], "f2_4": fm[1]}

        def mix(f, c, tag):                                   # net = tanh(avg), inp = relu(avg) of the two 128-channel halves
            c = c.contiguous().float()
            net, inp = f32(N, 128, f.shape[2], f.shape[3]), f32(N, 128, f.shape[2], f.shape[3])
            L.check(lib.ppms_ctx_mix(f.data_ptr(), c.data_ptr(), net.data_ptr(), inp.data_ptr(), N, f.shape[2] * f.shape[3], st()))
            feats["net_" + tag], feats["inp_" + tag] = net, inp

        h16, w16, h8, w8 = h // 4, w // 4, h // 2, w // 2
        f16 = []
        for f in fm:                                           # :649-652 avg_pool 4x4, then the SST block
            p = f32(N, C, h16, w16)
            L.check(lib.ppms_avgpool(f.data_ptr(), p.data_ptr(), N * C, h, w, 4, st()))
            f16.append(p)
        if self.sst is not None:
            f16 = list(self.sst(f16[0], f16[1], t))
        else:                                                  # forward_sst_block with attention_type=None: + positional encoding
            pe = self._pe(h16, w16, dev)
            for p in f16:
                L.check(lib.ppms_axpby(p.data_ptr(), pe.data_ptr(), p.data_ptr(), 1.0, 1.0, pe.numel(), p.numel(), st()))
        feats["f1_16"], feats["f2_16"] = f16
        if ctx_ready is not None:
            ctx_ready()
        mix(fm[0], c4, "4")
        mix(f16[0], c16, "16")
        for i, f in enumerate(fm):                             # :666-671 (avg_pool2 + interp(1/16)) / 2
            p = f32(N, C, h8, w8)
            L.check(lib.ppms_avgpool(f.data_ptr(), p.data_ptr(), N * C, h, w, 2, st()))
            q = bilinear(f16[i], (h8, w8), True)
            L.check(lib.ppms_axpby(p.data_ptr(), q.data_ptr(), p.data_ptr(), 0.5, 0.5, p.numel(), p.numel(), st()))
            feats[f"f{i + 1}_8"] = p
        mix(feats["f1_8"], c8, "8")
        return feats

    @torch.no_grad()
    def forward(self, image1: torch.Tensor, image2: torch.Tensor, flow_init=None, iters: int = 10, test_mode: bool = False, pipeline=None,
                diagnostics: Optional[dict] = None, output: Optional[OutputSpec] = None, crop=None, frames=None,
                rectify: Optional[StereoRectifier] = None):
        """PPMStereo.forward (ppmstereo.py:601-804): image (b, T, 3, H, W) in [0, 255], H, W multiples of 32 (b = 1: the device-resident
        cascade; b > 1: the reference's glue around the batched forward_update_block).  Float images as in the reference, or both uint8:
        with this package's encoders the bytes go through ONE kernel (ppms_video_ingest_u8) to the operands of the first convolutions --
        the same bits as ``forward(image1.float(), image2.float())``; with other encoder callables they are converted to float on the device.
        Or two ``YUVFrames`` on the device (decoded 4:2:0 frames: NV12 / I420): b = 1, T = their frame count; ONE kernel
        (ppms_video_ingest_yuv420) converts them and writes the same operands -- the bits of ``forward`` on their ``to_rgb_u8()``.
        test_mode: (flow_up, uncertainty), each (b, T, 1, H, W); else (predictions (D, b, T, 1, H, W), uncertainties).
        pipeline (test_mode only): a ``ClipPipeline`` -- the result is valid once ``pipeline.wait()`` has been called.
        diagnostics (b = 1): a dict that receives ``["attn_redo"]``, the per-scale fix-up accounting of the memory read-out (see ``cascade``).
        output (test_mode, b = 1): an ``OutputSpec`` -- the call returns a dict of device tensors (1, n, 1, H0, W0) under "disparity", "depth"
        and "uncertainties" as the spec asks, written by ONE ppms_disparity_egress launch behind the last iteration (no float32 full-resolution
        tensor is made); crop = (pad_left, pad_top, H0, W0) inside the frame (default: the whole frame), frames = (from, to) (default: all).
        rectify: a ``StereoRectifier`` -- the images are the RAW frames of an unrectified rig, two uint8 device tensors (1, T, 3, Hs, Ws) or two
        ``YUVFrames`` of its source size Hs x Ws; ONE kernel (ppms_video_ingest_u8_remap / ppms_video_ingest_yuv420_remap) undistorts, rectifies and
        writes the same operands -- the bits of ``forward`` on ``RectifyMap.apply_u8`` of each view's RGB bytes.  H, W above are then the rectified
        size, and so are the outputs'.  Float images raise TypeError (the remap reads decoded bytes), b > 1 NotImplementedError, another frame
        size than the maps' ValueError.  None (default): the calls above, launch for launch."""
        if flow_init is not None:
            raise NotImplementedError("flow_init: the reference's own path for it reads undefined state (ppmstereo.py:691-693, 763)")
        if rectify is not None:
            self._check_rectify("PPMStereo.forward", rectify, image1, image2)
        if self.fnet is None or self.cnet is None:
            raise RuntimeError("PPMStereo.forward needs the encoders: pass fnet= / cnet= (outside the hot path, SURVEY.md section 8 f3-f5)")
        egress = None
        if output is not None:
            if not test_mode:
                raise NotImplementedError("PPMStereo.forward: output= needs test_mode=True; the lists of intermediate predictions stay float32")
            egress = _EgressCall(output, crop, frames)
        elif crop is not None or frames is not None:
            raise ValueError("PPMStereo.forward: crop= and frames= select what output= writes; without output= they have no meaning")
        if isinstance(image1, YUVFrames) or isinstance(image2, YUVFrames):
            return self._forward_yuv(image1, image2, iters, test_mode, pipeline, diagnostics, egress, rectify)
        if rectify is not None:
            return self._forward_raw_u8(image1, image2, iters, test_mode, pipeline, diagnostics, egress, rectify)
        if torch.is_tensor(image1) and torch.is_tensor(image2) and (image1.dtype == torch.uint8) != (image2.dtype == torch.uint8):
            raise TypeError(f"PPMStereo.forward: image1 is {image1.dtype} and image2 is {image2.dtype}; both views must be uint8 or both floating point")
        b, T, c, h, w = image1.shape
        if b != 1 and pipeline is not None:
            raise NotImplementedError("PPMStereo.forward: a ClipPipeline overlaps consecutive batch-1 clips")
        if b != 1 and egress is not None:
            raise NotImplementedError("PPMStereo.forward: output= serves b = 1; the batched glue keeps float32 lists of predictions")
        images = (image1, image2)
        if image1.dtype == torch.uint8:
            if self._hip_encoders() and image1.is_cuda and image2.is_cuda:
                if image2.shape != image1.shape or c != 3:
                    raise ValueError(f"PPMStereo.forward: two uint8 videos of one shape (b, T, 3, H, W) expected, got {tuple(image1.shape)} and {tuple(image2.shape)}")
                images = _ByteFrames(image1.contiguous(), image2.contiguous(), 3 * h * w, b * T, h, w)
            else:                                              # encoder callables of the caller: they get what they get for a float video
                images = (image1.float(), image2.float())
        return self._forward_images(images, b, T, h, w, image1.device, iters, test_mode, pipeline, diagnostics, egress)

    @staticmethod
    def _check_rectify(who: str, rectify, *views) -> None:
        """What ``rectify=`` asks of the raw views (tensors (..., 3, Hs, Ws), ``YUVFrames`` or a ``YUVStereoVideo``); touches no device."""
        if not isinstance(rectify, StereoRectifier):
            raise TypeError(f"{who}: rectify must be a StereoRectifier, got {type(rectify).__name__}")
        for v in views:
            if isinstance(v, (YUVFrames, YUVStereoVideo)):
                rectify.check_source(who, v.height, v.width)
            elif torch.is_tensor(v):
                if v.dtype != torch.uint8:
                    raise TypeError(f"{who}: rectify= reads decoded bytes (uint8 frames or YUVFrames), got {v.dtype}; rectify float images before the call")
                if v.dim() != 5:
                    raise ValueError(f"{who}: a raw uint8 video has 5 dimensions, got {tuple(v.shape)}")
                rectify.check_source(who, v.shape[-2], v.shape[-1])
            else:
                raise TypeError(f"{who}: rectify= takes uint8 tensors or YUV frames, got {type(v).__name__}")

    def _forward_raw_u8(self, image1, image2, iters: int, test_mode: bool, pipeline, diagnostics, egress, rectify: StereoRectifier):
        """``forward`` on two raw uint8 videos (1, T, 3, Hs, Ws) on the device with ``rectify=`` (checked by ``_check_rectify``)."""
        b, T, c, hs, ws = image1.shape
        if image2.shape != image1.shape or c != 3:
            raise ValueError(f"PPMStereo.forward: two uint8 videos of one shape (1, T, 3, Hs, Ws) expected, got {tuple(image1.shape)} and {tuple(image2.shape)}")
        if b != 1:
            raise NotImplementedError("PPMStereo.forward: rectify= serves b = 1")
        L.require_gpu(image1, image2)
        rectify = rectify.to(image1.device)
        if self._hip_encoders():
            images = _ByteFrames(image1.contiguous(), image2.contiguous(), 3 * hs * ws, T, rectify.height, rectify.width, rectify=rectify)
            return self._forward_images(images, 1, T, rectify.height, rectify.width, image1.device, iters, test_mode, pipeline, diagnostics, egress)
        # encoder callables of the caller: the frames are rectified on the device and take the float path
        out = {} if egress is None else dict(output=egress.spec, crop=egress.crop, frames=egress.frames)
        left, right = rectify.apply_u8(image1[0], image2[0])
        return self.forward(left.float()[None], right.float()[None], iters=iters, test_mode=test_mode, pipeline=pipeline, diagnostics=diagnostics, **out)

    def _forward_yuv(self, image1, image2, iters: int, test_mode: bool, pipeline, diagnostics, egress=None, rectify: Optional[StereoRectifier] = None):
        """``forward`` on two ``YUVFrames`` on the device: b = 1, T = their frame count, the frame size as it is (with ``rectify``: its rectified size)."""
        if not (isinstance(image1, YUVFrames) and isinstance(image2, YUVFrames)):
            raise TypeError(f"PPMStereo.forward: image1 is {type(image1).__name__} and image2 is {type(image2).__name__}; both views must be YUVFrames or both tensors")
        video = YUVStereoVideo(image1, image2)
        L.require_gpu(image1.y, image2.y)
        out = {} if egress is None else dict(output=egress.spec, crop=egress.crop, frames=egress.frames)
        if rectify is not None:
            rectify = rectify.to(image1.device)
            if self._hip_encoders():
                return self._forward_images(_YUVPlanes(video, rectify=rectify), 1, len(video), rectify.height, rectify.width, image1.device, iters, test_mode,
                                            pipeline, diagnostics, egress)
            left, right = rectify.apply_u8(image1.to_rgb_u8(), image2.to_rgb_u8())
            return self.forward(left.float()[None], right.float()[None], iters=iters, test_mode=test_mode, pipeline=pipeline, diagnostics=diagnostics, **out)
        if self._hip_encoders():
            return self._forward_images(_YUVPlanes(video), 1, len(video), video.height, video.width, image1.device, iters, test_mode, pipeline, diagnostics,
                                        egress)
        # encoder callables of the caller: they get what they get for a float video
        return self.forward(image1.to_rgb_u8().float()[None], image2.to_rgb_u8().float()[None], iters=iters, test_mode=test_mode, pipeline=pipeline,
                            diagnostics=diagnostics, **out)

    def _hip_encoders(self) -> bool:
        """Both encoders are this package's: their plans take the first-layer operands ppms_video_ingest_u8 writes."""
        from .cnet import Feature
        from .encoder import BasicEncoder
        return isinstance(self.fnet, BasicEncoder) and isinstance(self.cnet, Feature)

    def _forward_images(self, images, b: int, T: int, h: int, w: int, dev, iters: int, test_mode: bool, pipeline, diagnostics, egress=None):
        """``forward`` behind its argument checks.  images: the two float videos (b, T, 3, h, w), or ``_ByteFrames`` / ``_YUVPlanes`` holding
        b * T decoded frames per view that one ingest kernel pads to h x w (``forward_batch_test`` hands a window over unpadded).
        egress (an ``_EgressCall``; test_mode, b = 1): the result is ``cascade``'s dict of output planes, each (1, n, 1, H0, W0)."""
        with torch.cuda.device(dev):
            # fnet (both views) and cnet (left view) depend on the images only and are chains of small launches that leave most of the chip
            # idle: cnet runs on a second stream beside fnet (whole call -3.5 ms at config 2); its outputs are handed to the caller's
            # stream with an event + record_stream
            cur = torch.cuda.current_stream(dev)
            if isinstance(images, (_ByteFrames, _YUVPlanes)):
                # bytes -> the operands of fnet's conv1 and cnet's stem, one launch on the caller's stream (ordered before the side stream's wait)
                fplan, cplan = self.fnet.plan(2 * b * T, h, w, dev), self.cnet.plan(b * T, h, w, dev)
                images.ingest(fplan.s0_view(), cplan.s0_view(), h, w)
                run_fnet = lambda: torch.split(fplan.run_filled(), b * T, dim=0)
                run_cnet = cplan.run_filled
                held = images.held()
            else:
                image1, image2 = images
                c = image1.shape[2]
                im1 = (2 * (image1 / 255.0) - 1.0).contiguous().reshape(b * T, c, h, w)
                im2 = (2 * (image2 / 255.0) - 1.0).contiguous().reshape(b * T, c, h, w)
                run_fnet = lambda: self.fnet([im1, im2])
                run_cnet = lambda: self.cnet(im1)
                held = (im1,)
            if self.parallel_encoders:
                side = self._encoder_stream(dev)
                side.wait_stream(cur)
                for t_ in held:
                    t_.record_stream(side)
                with torch.cuda.stream(side):
                    c4, c8, c16 = run_cnet()
                fmap1, fmap2 = run_fnet()
                for t_ in (c4, c8, c16):
                    if torch.is_tensor(t_):
                        t_.record_stream(cur)
                ready = {"done": False}

                def ctx_ready():                               # the pooling and the SST block run before this: they need fnet's output only
                    if not ready["done"]:
                        cur.wait_stream(side)
                        ready["done"] = True
            else:
                fmap1, fmap2 = run_fnet()
                c4, c8, c16 = run_cnet()
                ctx_ready = None
            if b == 1:
                feats = self.pre_loop(fmap1, fmap2, c4, c8, c16, T, ctx_ready)
            else:                                              # the glue in front of the loop is per clip (the SST block's time attention sees T frames)
                if ctx_ready is not None:
                    ctx_ready()
                per = [self.pre_loop(*(x[bi * T:(bi + 1) * T] for x in (fmap1, fmap2, c4, c8, c16)), T) for bi in range(b)]
                feats = {k: torch.cat([p_[k] for p_ in per]) for k in per[0]}
            preds, uncs = [], []
            if egress is not None:
                planes = self.cascade(feats, iters, T, test_mode=True, pipeline=pipeline, diagnostics=diagnostics, egress=egress)
                return {k: p[None] for k, p in planes.items()}
            self.cascade(feats, iters, T, preds, uncs, test_mode=test_mode, pipeline=pipeline if test_mode else None, diagnostics=diagnostics)
            if test_mode:
                return preds[-1].reshape(b, T, 1, h, w), uncs[-1].reshape(b, T, 1, h, w)
            return torch.stack(preds).reshape(-1, b, T, 1, h, w), torch.stack(uncs).reshape(-1, b, T, 1, h, w)

    @torch.no_grad()
    def forward_batch_test(self, batch_dict: Dict, kernel_size: int = 20, iters: int = 20, device=None, shard_ranks: bool = False,
                           diagnostics: bool = False, output: Optional[OutputSpec] = None, rectify: Optional[StereoRectifier] = None):
        """PPMStereo.forward_batch_test (ppmstereo.py:238-320): batch_dict["stereo_video"] (N, 2, 3, H, W) on the host;
        per window: InputPadder(divis_by=32), one host->device copy, forward(test_mode=True), unpad, one device->host copy;
        a uint8 video (host or device) is copied as bytes -- a quarter of the float video's -- and, with this package's encoders, padded and
        normalised inside ppms_video_ingest_u8: the same bits as for ``stereo_video.float()``;
        a ``YUVStereoVideo`` (decoded 8-bit 4:2:0 frames, NV12 or I420, host or device) is copied per window as its planes -- 1.5 bytes per
        pixel and view -- and converted, padded and normalised inside ppms_video_ingest_yuv420: the bits of the uint8 video of its
        ``to_rgb_u8()`` frames (10-bit formats, 4:2:2 / 4:4:4, interpolated chroma siting and b > 1 are not covered);
        windows of ``kernel_size`` frames every ``kernel_size // 2``, centre frames kept (:296-307).  Windows whose output the
        reference computes and then drops are not run.  Returns {"disparity", "uncertainties"}: (N, 1, H, W) CPU tensors.
        shard_ranks: under torch.distributed the windows are dealt round-robin over the ranks (independent units, no data-path
        collective) and the kept frames are gathered once at the end (``dist.gather_kept_frames``); every rank returns the video.
        diagnostics: the returned dict also has "attn_redo": the per-scale fix-up accounting of the memory read-out (see ``cascade``) summed
        over all windows (``shard_ranks``: over this rank's windows).  False (default): the two keys above, and no extra launch.
        output: an ``OutputSpec`` -- per window ONE ppms_disparity_egress launch writes the kept frames, cropped and converted, and only
        those are copied device -> host, straight into their slice of pinned (N, 1, H, W) results of the planes' dtypes (uint16 disparity and
        uint8 confidence: 3 bytes per pixel and kept frame, where the default path copies 8 for every frame of the window).  Returns
        {"disparity", "depth" when asked, "uncertainties" unless its format is None}.  Not with ``shard_ranks``.  None (default): the float32
        path above, launch for launch.
        rectify: a ``StereoRectifier`` -- the video holds the RAW frames of an unrectified rig, (N, 2, 3, Hs, Ws) uint8 or a ``YUVStereoVideo`` of
        its source size Hs x Ws.  Each window's raw bytes are copied as above, the maps once per call (6 bytes per rectified pixel and view), and
        ppms_video_ingest_u8_remap / ppms_video_ingest_yuv420_remap undistort, rectify, pad and normalise in the one ingest launch: the bits of
        the call on the uint8 video of ``RectifyMap.apply_u8``.  H x W of the results (and of the ``InputPadder``) is the rectified size.  A float
        video raises TypeError, another frame size than the maps' ValueError.  None (default): the paths above, launch for launch."""
        if output is not None:
            if not isinstance(output, OutputSpec):
                raise TypeError(f"forward_batch_test: output must be an OutputSpec, got {type(output).__name__}")
            if shard_ranks:
                raise NotImplementedError("forward_batch_test: output= with shard_ranks=True is not served: dist.gather_kept_frames moves float32")
        video = batch_dict["stereo_video"]
        if rectify is not None:
            self._check_rectify("forward_batch_test", rectify, video)
        num_ims = len(video)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if rectify is not None:
            rectify = rectify.to(dev)                             # the maps cross once per call, not once per window
        disp_preds, uncertainties = [], []
        diag = {} if diagnostics else None
        plan = window_plan(num_ims, kernel_size)
        if shard_ranks and torch.distributed.is_available() and torch.distributed.is_initialized():
            from . import dist as D
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
            mine_d, mine_u, first = [], [], 0
            firsts = []
            for start, stop, keep_from, keep_to in plan:          # first kept frame of every window in video coordinates
                firsts.append(start + keep_from)
            for wi, (start, stop, keep_from, keep_to) in enumerate(plan):
                if wi % world != rank:
                    continue
                d, u, padder = self._window_forward(video, start, stop, dev, iters, None, diag, rectify=rectify)   # one host -> device copy per window (see below)
                d, u = padder.unpad(d[0]), padder.unpad(u[0])               # (T, 1, H0, W0)
                mine_d.append((firsts[wi], d[keep_from:keep_to].abs()[:, :1]))
                mine_u.append((firsts[wi], u[keep_from:keep_to].abs()[:, :1]))
            H0, W0 = self._result_size(video, rectify)
            disp = D.gather_kept_frames(mine_d, num_ims, H0, W0)
            unc = D.gather_kept_frames(mine_u, num_ims, H0, W0)
            out = {"disparity": disp.cpu(), "uncertainties": unc.cpu()}
            if diag is not None:
                out["attn_redo"] = diag.get("attn_redo", {})
            return out
        # several windows: independent units -> software pipeline (ClipPipeline): window k + 1's encoders and small scales are enqueued
        # before window k's result is collected, and run under window k's 1/4 scale
        pipe = ClipPipeline(dev) if len(plan) > 1 else None
        pending = None
        if output is not None:
            H0, W0 = self._result_size(video, rectify)
            host = output.empty(num_ims, int(H0), int(W0), "cpu", pin_memory=True)           # allocated once; every window fills its slice

            def collect_planes(item):
                planes, handle, dst_from, dst_to = item
                if pipe is not None:
                    pipe.wait(handle)
                torch.cuda.current_stream(dev).synchronize()               # in front of the copy, as in collect() below
                for key, plane in planes.items():
                    host[key][dst_from:dst_to].copy_(plane[0])             # kept frames only, device -> their slice of the pinned result

            with torch.cuda.device(dev):
                for start, stop, keep_from, keep_to, dst_from, dst_to in egress_plan(plan):
                    planes = self._window_forward(video, start, stop, dev, iters, pipe, diag, output, (keep_from, keep_to), rectify=rectify)
                    item = (planes, None if pipe is None else pipe.last, dst_from, dst_to)
                    if pending is not None:
                        collect_planes(pending)
                    pending = item
                collect_planes(pending)
            if diag is not None:
                host["attn_redo"] = diag.get("attn_redo", {})
            return host

        def collect(item):
            d, u, handle, padder, keep_from, keep_to = item
            if pipe is not None:
                pipe.wait(handle)
            # device -> host.  The stream is synchronised FIRST (a spinning wait): a pageable copy issued while the clip's ~900 launches are
            # still queued blocks inside the runtime on an interrupt-driven wait, and on a loaded host (the GPU boxes: load average 50-60)
            # the thread was rescheduled 50-150 ms late in every other call (whole call 50 / 100 / 195 ms alternating; with the
            # synchronisation in front the copy finds an idle stream: 49-50 ms every time, tools/whole_call_probe.py)
            du = torch.cat([padder.unpad(d[0])[:, None], padder.unpad(u[0])[:, None]])                        # one copy for both results
            torch.cuda.current_stream(du.device).synchronize()
            du = du.cpu()
            d, u = du[:du.shape[0] // 2], du[du.shape[0] // 2:]
            disp_preds.append(d[keep_from:keep_to])
            uncertainties.append(u[keep_from:keep_to])

        with torch.cuda.device(dev):
            for start, stop, keep_from, keep_to in plan:
                d, u, padder = self._window_forward(video, start, stop, dev, iters, pipe, diag, rectify=rectify)
                item = (d, u, None if pipe is None else pipe.last, padder, keep_from, keep_to)
                if pending is not None:
                    collect(pending)
                pending = item
            collect(pending)
        out = {"disparity": torch.cat(disp_preds).squeeze(1).abs()[:, :1], "uncertainties": torch.cat(uncertainties).squeeze(1).abs()[:, :1]}
        if diag is not None:
            out["attn_redo"] = diag.get("attn_redo", {})
        return out


def _result_size(video, rectify: Optional[StereoRectifier]):
    """(H0, W0) of forward_batch_test's results: the rectified size, or the video's own."""
    if rectify is not None:
        return rectify.height, rectify.width
    return (video.height, video.width) if isinstance(video, YUVStereoVideo) else video.shape[-2:]


PPMStereo._result_size = staticmethod(_result_size)


def _window_forward(self, video, start: int, stop: int, dev, iters: int, pipe, diag, output: Optional[OutputSpec] = None, keep=None,
                    rectify: Optional[StereoRectifier] = None):
    """One window of forward_batch_test: frames [start, stop) of the (N, 2, 3, H0, W0) video or the YUVStereoVideo -> (disparity, uncertainty) of the padded
    window, each (1, T, 1, H, W), and the InputPadder that crops them back.  output (an OutputSpec): the window's egress launch crops with that
    padder's geometry and writes the window-local frames keep = (from, to); the result is then the dict of planes, each (1, n, 1, H0, W0).
    rectify (a StereoRectifier on dev): the video holds raw frames of its source size; H0 x W0, and so the padder, is its rectified size."""
    def egress(padder):
        if output is None:
            return None
        pad_left, pad_top, _, _ = padder.geometry()
        return _EgressCall(output, (pad_left, pad_top, padder.ht, padder.wd), keep)

    # host -> device: ONE copy of the window's contiguous (T, 2, 3, H, W) block; the two views are split and padded on the
    # device (slicing a view out on the host first costs a host-side copy of each view, padding there another one)
    win = video[start:stop].to(dev)
    if isinstance(win, YUVStereoVideo):
        if self._hip_encoders():
            # the planes stay as the decoder left them: ppms_video_ingest_yuv420 converts, and pads by clamping its source coordinate
            padder = InputPadder(_result_size(win, rectify), divis_by=32)
            pad_left, pad_top, H, W = padder.geometry()
            planes = _YUVPlanes(win, pad_left, pad_top, rectify)
            if output is not None:
                return self._forward_images(planes, 1, len(win), H, W, dev, iters, True, pipe, diag, egress(padder))
            d, u = self._forward_images(planes, 1, len(win), H, W, dev, iters, True, pipe, diag)
            return d, u, padder
        rgb = win.left.to_rgb_u8(), win.right.to_rgb_u8()
        if rectify is not None:
            rgb = rectify.apply_u8(*rgb)
        win = torch.stack(rgb, dim=1).float()                   # encoder callables of the caller: the float path
    elif win.dtype == torch.uint8:
        if win.dim() != 5 or win.shape[1] != 2 or win.shape[2] != 3:
            raise ValueError(f"forward_batch_test: a uint8 stereo_video is (N, 2, 3, H, W), got {tuple(video.shape)}")
        if self._hip_encoders():
            # the bytes stay as they are: ppms_video_ingest_u8 reads both views out of the block and pads by clamping its source coordinate
            win = win.contiguous()
            T, H0, W0 = win.shape[0], win.shape[3], win.shape[4]
            stride = 6 * H0 * W0
            if rectify is not None:                              # the block holds raw frames; what is padded is the rectified frame
                H0, W0 = rectify.height, rectify.width
            padder = InputPadder((H0, W0), divis_by=32)
            pad_left, pad_top, H, W = padder.geometry()
            frames = _ByteFrames(win[:, 0], win[:, 1], stride, T, H0, W0, pad_left, pad_top, rectify)
            if output is not None:
                return self._forward_images(frames, 1, T, H, W, dev, iters, True, pipe, diag, egress(padder))
            d, u = self._forward_images(frames, 1, T, H, W, dev, iters, True, pipe, diag)
            return d, u, padder
        if rectify is not None:
            win = torch.stack(rectify.apply_u8(win[:, 0], win[:, 1]), dim=1)
        win = win.float()                                        # encoder callables of the caller: the float path from here on
    left, right = win[:, 0], win[:, 1]
    padder = InputPadder(left.shape, divis_by=32)
    left, right = padder.pad(left, right)
    if output is not None:
        return self.forward(left[None], right[None], iters=iters, test_mode=True, pipeline=pipe, diagnostics=diag, output=output,
                            crop=egress(padder).crop, frames=keep)
    d, u = self.forward(left[None], right[None], iters=iters, test_mode=True, pipeline=pipe, diagnostics=diag)
    return d, u, padder


PPMStereo._window_forward = _window_forward


def window_plan(num_ims: int, kernel_size: int = 20):
    """Sliding-window schedule of PPMStereo.forward_batch_test (ppmstereo.py:242-310): list of
    (start, stop, keep_from, keep_to) with keep_* window-local.  Trailing windows whose output the reference
    discards (:296) are not scheduled at all."""
    stride = kernel_size // 2
    if kernel_size > num_ims:
        return [(0, num_ims, 0, num_ims)]
    plan = []
    for i in range(0, num_ims, stride):
        n = min(i + kernel_size, num_ims) - i
        if plan and n >= stride:
            plan.append((i, i + n, stride // 2, n if n < kernel_size else n + (-stride // 2)))
        elif not plan:
            plan.append((i, i + n, 0, n + (-stride // 2)))
    return plan


def egress_plan(plan):
    """``window_plan`` with the destination of every window's kept frames: (start, stop, keep_from, keep_to, dst_from, dst_to) -- the egress
    launch of the window writes its frames [keep_from, keep_to), and they are frames [dst_from, dst_to) of the video."""
    return [(start, stop, keep_from, keep_to, start + keep_from, start + keep_to) for start, stop, keep_from, keep_to in plan]


def shard_windows(plan, rank: int, world: int):
    """Window-level sharding across GPUs (SURVEY.md section 8e level 1): windows are independent units; rank r takes
    windows r, r+world, ...  No data-path collective; the kept disparities are gathered once at the end."""
    return [w for i, w in enumerate(plan) if i % world == rank]
