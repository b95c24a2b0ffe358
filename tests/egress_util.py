"""What the egress test files share (tests/test_egress*.py without a device, tests/test_gpu_egress*.py with one): the library, the header's argument
lists, calls of the three entry points on fake pointers over one default geometry, the refusal test's body, random grids -- and on the GPU side
synthetic engine state, the reference on the host, destinations, one launch and one check, the rig's constants and the model (ingest_util's).  The oracles (the
float64 restatements, the points-at-valid-pixels test) stay in the file of the feature they define; ``OutputSpec.reference`` is what they test."""
import ctypes
import math
import os
import re

import pytest
import torch

from ingest_util import DEV, model, rand_u8  # noqa: F401  (the video tests of both doors share the device, the model fixture and the random bytes)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.engine import bilinear
from ppmstereo_amd.ppmstereo import OutputSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return L.load()


def header_args(name):
    """The argument list of `name` as include/ppms.h declares it."""
    src = open(os.path.join(ROOT, "include", "ppms.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppms.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- argument refusal: frames [1, 3) of T = 3, the 37 x 50 crop at (13, 7) of 64 x 64; u16 / u16 / u8 planes with pitches wider than the row, an
# ---- "xyz" f32 points plane whose pitch (604) is wider than the row's 600 bytes; Q = identity and both gates on.  Pointers into device memory are
# ---- never dereferenced on the host: every check comes before the launch ------------------------------------------------------------------------
GEOMETRY = dict(flow=0x100000, unc=0x200000, T=3, H=64, W=64, frame0=1, n_frames=2, pad_left=7, pad_top=13, H0=37, W0=50)
PLANES = {"disparity": dict(ptr=0x300000, frame_stride=37 * 102, pitch=102, format=L.FMT_U16, reserved=0),
          "depth": dict(ptr=0x400000, frame_stride=37 * 106, pitch=106, format=L.FMT_U16, reserved=0),
          "uncertainty": dict(ptr=0x500000, frame_stride=37 * 53, pitch=53, format=L.FMT_U8, reserved=0),
          "points": dict(ptr=0x600000, frame_stride=37 * 604, pitch=604, format=L.FMT_F32, reserved=0)}
IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


def _q(i, v):
    return [v if j == i else x for j, x in enumerate(IDENTITY)]


def _enter(lib, entry, out, null_out, geometry):
    g = {**GEOMETRY, **geometry}
    return getattr(lib, entry)(g["flow"] or None, g["unc"] or None, g["T"], g["H"], g["W"], g["frame0"], g["n_frames"], g["pad_left"], g["pad_top"], g["H0"],
                               g["W0"], None if null_out else ctypes.byref(out), None)


def _split(kw):
    """kw -> (the call's geometry, the planes with their "<plane>_<field>" = value changes)"""
    planes = {k: dict(v) for k, v in PLANES.items()}
    for key in [k for k in kw if k not in GEOMETRY]:
        plane, field = key.split("_", 1)
        planes[plane][field] = kw.pop(key)
    return kw, planes


def _egress(planes, given, disp_scale, fb, depth_scale, min_disp):
    pl = {k: L.EgressPlane(**{**v, "ptr": v["ptr"] or None}) if k in given else L.EgressPlane(None, 0, 0, 0, 0) for k, v in planes.items()}
    return L.Egress(pl["disparity"], pl["depth"], pl["uncertainty"], disp_scale, fb, depth_scale, min_disp), pl["points"]


def call_disparity(lib, planes=("disparity", "depth", "uncertainty"), null_out=False, disp_scale=256.0, fb=500.0, depth_scale=1000.0, min_disp=0.25, **kw):
    """ppms_disparity_egress.  kw: the geometry's entries and "<plane>_<field>" = value."""
    geometry, fields = _split(kw)
    return _enter(lib, "ppms_disparity_egress", _egress(fields, planes, disp_scale, fb, depth_scale, min_disp)[0], null_out, geometry)


def call_scene(lib, planes=("disparity", "depth", "uncertainty", "points"), null_out=False, disp_scale=256.0, fb=500.0, depth_scale=1000.0, min_disp=0.25,
               q=IDENTITY, max_uncertainty=0.5, max_depth=80.0, comps=3, reserved=0, **kw):
    """ppms_scene_egress.  kw: as call_disparity's."""
    geometry, fields = _split(kw)
    base, points = _egress(fields, planes, disp_scale, fb, depth_scale, min_disp)
    out = L.Egress3D(base, points, (ctypes.c_float * 16)(*q), max_uncertainty, max_depth, comps, reserved)
    return _enter(lib, "ppms_scene_egress", out, null_out, geometry)


def call_cloud(lib, null_out=False, records=0x300000, frame_stride=12008, capacity=1000, index=0x400000, index_frame_stride=4004, counts=0x500000,
               block_counts=0x600000, block_counts_len=4, q=IDENTITY, min_disp=0.25, max_uncertainty=0.5, max_depth=80.0, format=0, components=3, reserved=0,
               **geometry):
    """ppms_cloud_egress: "xyz" f32 records with a capacity of 1000 and a gap between the frames, an index."""
    out = L.Cloud(records or None, frame_stride, capacity, index or None, index_frame_stride, counts or None, block_counts or None, block_counts_len,
                  (ctypes.c_float * 16)(*q), min_disp, max_uncertainty, max_depth, format, components, reserved)
    return _enter(lib, "ppms_cloud_egress", out, null_out, geometry)


def bad_ids(bad):
    return [about.replace(" ", "_") + ":" + ",".join(k if k == "q" else f"{k}={v}" for k, v in b.items()) for about, b in bad]


def refused(lib, call, entry, about, bad):
    """The call with ``bad``, the one thing that is wrong with it, returns EINVAL with a message that names the entry point and speaks of ``about``."""
    lib.ppms_mem_attn_splits(3, 3, 256, 1)                      # (a successful call in between: the message below is this call's)
    assert call(lib, **bad) == EINVAL, bad
    msg = lib.ppms_last_error()
    assert msg and entry.encode() in msg and about.encode() in msg, (bad, msg)


CAL_700 = dict(focal_px=700.0, baseline=0.25)               # the calibration of the OutputSpec validation tests


def grid_inputs(H=24, W=40, seed=7, min_disp=0.5):
    """(2, 1, H, W) disparities in (0, 100) with both signs, a tenth below min_disp, a twentieth NaN, some exact zeros; uncertainties in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * H * W
    d = (torch.rand(n, generator=g) * 99.0 + 1.0) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    pick = torch.randperm(n, generator=g)
    d[pick[:n // 10]] = torch.rand(n // 10, generator=g) * min_disp * 0.99
    d[pick[n // 10:n // 10 + n // 20]] = math.nan
    d[pick[n // 10 + n // 20:n // 10 + n // 20 + 8]] = 0.0
    return d.reshape(2, 1, H, W), torch.rand(2, 1, H, W, generator=g)


# ---- with a device: engine state, the reference on the host, destinations, the launch and the check, the rig, the model ---------------------------
FMT = {"f32": (L.FMT_F32, torch.float32, 4), "f16": (L.FMT_F16, torch.float16, 2), "u16": (L.FMT_U16, torch.uint16, 2), "u8": (L.FMT_U8, torch.uint8, 1)}
KEYS = ("disparity", "depth", "uncertainties")
ALL = KEYS + ("points",)
NO_PLANE = L.EgressPlane(None, 0, 0, 0, 0)
F, B = 721.5377, 0.54                                        # fb = 389.6: with d in [0, 400), max_depth = 5 gates d < 78
Q = OutputSpec.q_matrix(F, B, 24.3, 17.6)
GATES = dict(max_uncertainty=0.7, max_depth=5.0)
RIG_CAL = dict(focal_px=F, baseline=B, min_disp=0.25)
POISON = 0x5A
COUNT_POISON = int.from_bytes(bytes([POISON] * 4), "little")


def same(a, b):
    """Equal dtype, shape and values; NaN equals NaN."""
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        return False
    if a.dtype.is_floating_point:
        a, b = (torch.where(x.isnan(), torch.full_like(x, -1.0), x) for x in (a, b))
        return torch.equal(a, b)
    return torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a, b.view(torch.int16) if b.dtype == torch.uint16 else b)


def same_results(a, b, keys=("disparity", "uncertainties")):
    return all(same(a[k], b[k]) for k in keys)


def engine_state(T, H, Wd, seed, min_disp=0.25):
    """flow_up (T, 2, H, W): channel 0 = magnitudes in [0, 400) with both signs, exact zeros, values below min_disp, NaN and exact u16 ties k / 512
    sprinkled in; channel 1 = another pattern (a wrong channel stride shows).  unc (T, H/4, W/4) in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    n = T * H * Wd
    d = torch.rand(n, generator=g) * 400.0
    d = d * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    pick = torch.randperm(n, generator=g)
    q = n // 16
    d[pick[:q]] = 0.0
    d[pick[q:2 * q]] = torch.rand(q, generator=g) * min_disp * torch.where(torch.rand(q, generator=g) < 0.5, -1.0, 1.0)
    d[pick[2 * q:3 * q]] = float("nan")
    d[pick[3 * q:4 * q]] = (2 * torch.randint(0, 60000, (q,), generator=g) + 1).float() / 512.0 * torch.where(torch.rand(q, generator=g) < 0.5, -1.0, 1.0)
    flow = torch.stack([d.reshape(T, H, Wd), 1000.0 + torch.rand(T, H, Wd, generator=g)], dim=1).contiguous()
    unc = torch.rand(T, H // 4, Wd // 4, generator=g)
    return flow.to(DEV), unc.to(DEV)


def expected(spec, flow, unc, f0, f1, left, top, h0, w0):
    """OutputSpec.reference on the sliced flow_up and on ppms_bilinear's 4x upsampling of unc -- evaluated on the host, where torch's fp32
    division and conversions are the IEEE ones beyond doubt -> CPU tensors."""
    T, _, H, Wd = flow.shape
    up = bilinear(unc.view(T, 1, H // 4, Wd // 4), (H, Wd), False)
    cut = lambda x: x[f0:f1, :1, top:top + h0, left:left + w0].cpu()
    return spec.reference(cut(flow), cut(up))


def all_kinds(spec, want, flow, unc, f0, n, left, top, h0, w0):
    """On the reference side: valid pixels, pixels the uncertainty gate takes, pixels the depth gate takes, and NaN disparities all occur."""
    T, _, H, Wd = flow.shape
    cut = lambda x: x[f0:f0 + n, 0, top:top + h0, left:left + w0].abs().cpu()
    d, u = cut(flow), cut(bilinear(unc.view(T, 1, H // 4, Wd // 4), (H, Wd), False))
    if "points" in want:
        ok = ~want["points"][..., 2].float().isnan()
    else:
        ok = want["depth"][:, 0].to(torch.int32) != 0 if want["depth"].dtype == torch.uint16 else ~want["depth"][:, 0].float().isinf()
    vd, vu = d >= spec.min_disp, u <= spec.max_uncertainty
    return bool(ok.any() and (vd & ~vu).any() and (vd & vu & ~ok).any() and d.isnan().any() and (~vd & ~d.isnan()).any() and not (ok & ~(vd & vu)).any())


class Dest:
    """A byte buffer of ``frames`` output frames with a pitch, filled with a non-zero pattern; the launch writes n frames from frame ``first`` on.
    (The points' Dest is a plane of w0 * C elements per row.)"""

    def __init__(self, fmt, frames, h0, w0, pitch_extra=0, first=0, frame_gap=0):
        self.fmt, self.h0, self.w0, self.first = fmt, h0, w0, first
        self.es = FMT[fmt][2]
        self.pitch = w0 * self.es + pitch_extra
        self.frame_stride = h0 * self.pitch + frame_gap
        size = frames * self.frame_stride
        self.pattern = (torch.arange(size, device=DEV) % 251 + 1).to(torch.uint8)
        self.buf = self.pattern.clone()

    def plane(self):
        return L.EgressPlane(self.buf.data_ptr() + self.first * self.frame_stride, self.frame_stride, self.pitch, FMT[self.fmt][0], 0)

    def region(self, t, n):
        return torch.as_strided(t, (n, self.h0, self.w0 * self.es), (self.frame_stride, self.pitch, 1), self.first * self.frame_stride)

    def written(self, n):
        """(n, 1, h0, w0) tensor of the plane's dtype: what lies in the n frames' rows."""
        return self.region(self.buf, n).contiguous().view(FMT[self.fmt][1]).reshape(n, 1, self.h0, self.w0).cpu()

    def rest_untouched(self, n):
        """Every byte outside the n frames' rows -- between rows, between frames, the frames before and after -- still holds the pattern."""
        mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.region(mask, n).fill_(True)
        return torch.equal(self.buf[~mask], self.pattern[~mask])

    def untouched(self):
        return torch.equal(self.buf, self.pattern)


def planes_struct(spec, dests, scene=False):
    """dests: {key: Dest or None} -> the L.Egress of ppms_disparity_egress or, scene, the L.Egress3D of ppms_scene_egress with Q, the gates and the
    component count as the spec hands them over."""
    pl = [dests[k].plane() if dests.get(k) is not None else NO_PLANE for k in ALL]
    base = L.Egress(pl[0], pl[1], pl[2], spec.disp_scale, spec.fb, spec.depth_scale, spec.min_disp)
    if not scene:
        return base
    rest = spec.scene_struct({})
    return L.Egress3D(base, pl[3], rest.q, rest.max_uncertainty, rest.max_depth, rest.points_components, 0)


def planes_match(dests):
    """check's comparison for {key: Dest}: every destination holds the reference's plane in its n frames' rows and the pattern everywhere else."""
    def compare(want, n, h0, w0):
        for key, dest in dests.items():
            got = dest.written(n)
            assert same(got.reshape(n, h0, w0, -1) if key == "points" else got, want[key].contiguous()), key
            assert dest.rest_untouched(n), key
    return compare


class CloudDest:
    """Poisoned destinations of ``frames`` frames, written from frame ``first`` on: records of ``capacity`` per frame with ``gap`` bytes between
    the frames, starting ``lead`` bytes into their allocation; indices likewise; counts."""

    def __init__(self, fmt, C, frames, capacity, first=0, gap=0, index_gap=0, lead=0, index=True):
        self.dtype, self.C, self.frames, self.capacity, self.first, self.lead = FMT[fmt][1], C, frames, capacity, first, lead
        self.rb = FMT[fmt][2] * C
        self.frame_stride, self.index_frame_stride = capacity * self.rb + gap, capacity * 4 + index_gap
        self.records = torch.full((lead + frames * self.frame_stride,), POISON, dtype=torch.uint8, device=DEV)
        self.index = torch.full((frames * self.index_frame_stride,), POISON, dtype=torch.uint8, device=DEV) if index else None
        self.counts = torch.full((frames,), COUNT_POISON, dtype=torch.int32, device=DEV)

    def struct(self, spec, n, h0, w0):
        self.workspace = torch.full((L.load().ppms_cloud_egress_workspace(n, h0, w0),), COUNT_POISON, dtype=torch.int32, device=DEV)
        st = spec.cloud_struct({}, self.workspace)                # Q, min_disp, the gates, the format and the component count as the spec hands them over
        st.records, st.frame_stride, st.capacity = self.records.data_ptr() + self.lead + self.first * self.frame_stride, self.frame_stride, self.capacity
        if self.index is not None:
            st.index, st.index_frame_stride = self.index.data_ptr() + self.first * self.index_frame_stride, self.index_frame_stride
        st.counts = self.counts.data_ptr() + 4 * self.first
        return st

    def check(self, n, want, capacity_hit=False):
        """Frame f of the launch holds the first min(count, capacity) records and indices of the reference's and poison from there to the next
        frame's first byte; the other frames' bytes and counts are poison; the counts are the reference's (full) numbers."""
        rec, idx, counts = self.records.cpu(), None if self.index is None else self.index.cpu(), self.counts.cpu()
        assert (rec[:self.lead] == POISON).all()
        hit = False
        for fr in range(self.frames):
            f = fr - self.first
            r = rec[self.lead + fr * self.frame_stride:self.lead + (fr + 1) * self.frame_stride]
            i = None if idx is None else idx[fr * self.index_frame_stride:(fr + 1) * self.index_frame_stride]
            if not 0 <= f < n:
                assert (r == POISON).all() and (i is None or (i == POISON).all()) and int(counts[fr]) == COUNT_POISON, fr
                continue
            count = int(want["cloud_counts"][f])
            assert int(counts[fr]) == count == want["cloud"][f].shape[0], (fr, int(counts[fr]), count)
            k = min(count, self.capacity)
            hit |= count > self.capacity
            assert want["cloud"][f].dtype == self.dtype and want["cloud"][f].shape[1] == self.C
            assert torch.equal(r[:k * self.rb], want["cloud"][f][:k].contiguous().view(torch.uint8).flatten()), fr
            assert (r[k * self.rb:] == POISON).all(), fr
            if i is not None:
                assert torch.equal(i[:4 * k], want["cloud_index"][f][:k].contiguous().view(torch.uint8).flatten()), fr
                assert (i[4 * k:] == POISON).all(), fr
        assert hit == capacity_hit


def launch(entry, out, flow, unc, f0, n, left, top, h0, w0):
    """One of the three entry points on the engine state, frames [f0, f0 + n) and the h0 x w0 crop at (top, left), with its struct ``out``."""
    T, _, H, Wd = flow.shape
    with torch.cuda.device(DEV):
        L.check(getattr(L.load(), entry)(flow.data_ptr(), unc.data_ptr(), T, H, Wd, f0, n, left, top, h0, w0, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()


def check(entry, out, compare, spec, flow, unc, f0, n, left, top, h0, w0, kinds=False):
    """The reference on the host, the launch, then ``compare(want, n, h0, w0)``: the comparison of the destinations' kind (planes_match(dests),
    CloudDest.check behind a lambda).  kinds: every kind of pixel occurs on the reference side (all_kinds)."""
    want = expected(spec, flow, unc, f0, f0 + n, left, top, h0, w0)
    launch(entry, out, flow, unc, f0, n, left, top, h0, w0)
    compare(want, n, h0, w0)
    assert not kinds or all_kinds(spec, want, flow, unc, f0, n, left, top, h0, w0)
    return want


def model_refuses(model, monkeypatch, spec):
    """output=spec where float32 lists or gathers remain: training mode, b = 2, sharded ranks."""
    v = rand_u8((1, 2, 3, 64, 256), 51).to(DEV)
    with pytest.raises(NotImplementedError):
        model.forward(v, v, iters=2, test_mode=False, output=spec)
    with pytest.raises(NotImplementedError):
        model.forward(v.expand(2, -1, -1, -1, -1), v.expand(2, -1, -1, -1, -1), iters=2, test_mode=True, output=spec)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError):
        model.forward_batch_test({"stereo_video": rand_u8((3, 2, 3, 60, 250), 52)}, kernel_size=20, iters=2, shard_ranks=True, output=spec)
