"""What the normals test files share (tests/test_normals_out.py without a device, tests/test_gpu_normals_out.py with one): the surface state --
egress_util.engine_state's uniformly random disparities would let the jump gate take nearly every neighbour --, the stencil kinds on the reference
side, the float64 restatement of the definition, calls of the two entry points on fake pointers over egress_util's geometry, and on the GPU side the
reference on the host and the launches."""
import ctypes
import math

import torch

from egress_util import DEV, GEOMETRY, IDENTITY, B, F, Q, bilinear  # noqa: F401
from ppmstereo_amd import _lib as L
from ppmstereo_amd.ppmstereo import OutputSpec

TILE_H, TILE_W = 16, 128                                     # normals_egress_kernel's tile (csrc/normals_egress.hip: NT_H, NT_W)
Q_REVERSED = OutputSpec.q_matrix(F, -B, 24.3, 17.6)          # the baseline's sign reversed: every point negated, every normal takes the flip
N_RIG = dict(min_disp=0.25, Q=Q)
N_GATES = dict(max_uncertainty=0.7, max_depth=12.0)          # fb = 389.6 and d in 20 .. 60: Z in 6.5 .. 19.5, the depth gate takes d < 32.5
A_CROP = (1, 2, 7, 13, 37, 50)                               # (f0, n, left, top, h0, w0): frames [1, 3), the 37 x 50 crop at (13, 7) of 64 x 64


# ---- argument refusal on fake pointers (egress_util's GEOMETRY; pointers into device memory are never dereferenced on the host) -----------------
def _enter(lib, entry, out, null_out, geometry, *extra):
    g = {**GEOMETRY, **geometry}
    return getattr(lib, entry)(g["flow"] or None, g["unc"] or None, g["T"], g["H"], g["W"], g["frame0"], g["n_frames"], g["pad_left"], g["pad_top"], g["H0"],
                               g["W0"], None if null_out else ctypes.byref(out), *extra, None)


def call_normals(lib, null_out=False, ptr=0x300000, frame_stride=37 * 604, pitch=604, format=0, plane_reserved=0, q=IDENTITY, min_disp=0.25,
                 max_uncertainty=0.5, max_depth=80.0, max_jump=0.05, reserved=0, **geometry):
    """ppms_normals_egress: an f32 plane whose pitch (604) is wider than the row's 600 bytes, Q = identity, every gate on."""
    out = L.Normals(L.EgressPlane(ptr or None, frame_stride, pitch, format, plane_reserved), (ctypes.c_float * 16)(*q), min_disp, max_uncertainty,
                    max_depth, max_jump, reserved)
    return _enter(lib, "ppms_normals_egress", out, null_out, geometry)


def call_cloud_normals(lib, null_out=False, records=0x300000, frame_stride=24016, capacity=1000, index=0x400000, index_frame_stride=4004, counts=0x500000,
                       block_counts=0x600000, block_counts_len=8, q=IDENTITY, min_disp=0.25, max_uncertainty=0.5, max_depth=80.0, format=0, components=6,
                       reserved=0, normals=dict(), colour=None, null_normals=False, **geometry):
    """ppms_cloud_egress_normals: "xyzn" f32 records with a capacity of 1000 and a gap between the frames, an index; the normals plane as
    call_normals', no colour plane.  normals / colour: the fields of that plane's struct that differ (colour: None = a NULL pointer)."""
    out = L.Cloud(records or None, frame_stride, capacity, index or None, index_frame_stride, counts or None, block_counts or None, block_counts_len,
                  (ctypes.c_float * 16)(*q), min_disp, max_uncertainty, max_depth, format, components, reserved)
    nrm = {**dict(ptr=0x700000, frame_stride=37 * 604, pitch=604, format=0, reserved=0), **normals}
    nrm = L.EgressPlane(nrm["ptr"] or None, nrm["frame_stride"], nrm["pitch"], nrm["format"], nrm["reserved"])
    col = None
    if colour is not None:
        col = {**dict(ptr=0x800000, frame_stride=37 * 200, pitch=200, format=L.FMT_BGRA8, reserved=0), **colour}
        col = ctypes.byref(L.EgressPlane(col["ptr"] or None, col["frame_stride"], col["pitch"], col["format"], col["reserved"]))
    return _enter(lib, "ppms_cloud_egress_normals", out, null_out, geometry, None if null_normals else ctypes.byref(nrm), col)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------
def surface_state(T=3, H=64, W=64, seed=5, min_disp=0.25, noise=0.02, holes=True):
    """CPU tensors flow_up (T, 2, H, W) and unc (T, H/4, W/4).  Channel 0 is a surface: per frame t the plane d = 20 + 0.35 x + 0.2 y + 3 t; for
    x >= W/2 + y // 8 the plane 60 - 0.3 x + 0.15 y (a slanted step edge); for y >= 5H/8 and x < W/3 the constant 33 (a fronto-parallel patch);
    plus noise * rand.  holes: 1/24 of the pixels NaN, 1/24 below min_disp, eight exact zeros.  Random signs.  Channel 1 holds another pattern
    (a wrong channel stride shows); unc is random in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    frames = []
    for t in range(T):
        d = 20.0 + 0.35 * x + 0.2 * y + 3.0 * t
        d = torch.where(x >= W // 2 + y // 8, 60.0 - 0.3 * x + 0.15 * y, d)
        frames.append(torch.where((y >= 5 * H // 8) & (x < W // 3), torch.full_like(d, 33.0), d))
    d = (torch.stack(frames) + noise * torch.rand(T, H, W, generator=g)).flatten()
    n = d.numel()
    if holes:
        pick, k = torch.randperm(n, generator=g), n // 24
        d[pick[:k]] = math.nan
        d[pick[k:2 * k]] = torch.rand(k, generator=g) * min_disp * 0.99
        d[pick[2 * k:2 * k + 8]] = 0.0
    d = d * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    flow = torch.stack([d.reshape(T, H, W), 1000.0 + torch.rand(T, H, W, generator=g)], dim=1).contiguous()
    return flow, torch.rand(T, H // 4, W // 4, generator=g)


def crop(x, f0, n, left, top, h0, w0):
    """(n, 1, h0, w0): the frames and the crop of a (T, C, H, W) tensor's channel 0."""
    return x[f0:f0 + n, :1, top:top + h0, left:left + w0]


def stencil_kinds(spec, d, u=None):
    """The 4 x 4 table of pixel counts by stencil kind on the reference side -- [horizontal][vertical], each 0 = both neighbours usable, 1 = only
    the plus side (right / down), 2 = only the minus side (left / up), 3 = neither -- and the normals' validity.  Step 1 of the definition,
    restated on the reference's own fp32 points (NaN where invalid: a comparison with one is false)."""
    kw = dict(points="f32", Q=spec.Q, min_disp=spec.min_disp, max_uncertainty=spec.max_uncertainty, max_depth=spec.max_depth, uncertainty=None)
    z = OutputSpec(**kw).reference(d, u)["points"][..., 2]
    ok = ~z.isnan()
    h, w = z.shape[-2:]

    def usable(dy, dx):
        nb = torch.full_like(z, math.nan)
        nb[..., max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = z[..., max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)]
        near = (nb - z).abs() <= torch.tensor(spec.normal_max_jump, dtype=torch.float32) * z.abs() if spec.normal_max_jump is not None else True
        return ok & ~nb.isnan() & near

    kind = lambda plus, minus: torch.where(plus & minus, 0, torch.where(plus, 1, torch.where(minus, 2, 3)))
    hk, vk = kind(usable(0, 1), usable(0, -1)), kind(usable(1, 0), usable(-1, 0))
    table = torch.zeros(4, 4, dtype=torch.int64)
    for a in range(4):
        for b in range(4):
            table[a, b] = int(((hk == a) & (vk == b) & ok).sum())
    return table, ok & (hk < 3) & (vk < 3)


def every_kind(table, least=1):
    """The 15 kinds that can occur next to a valid centre do (none x none needs an isolated pixel; the surface has none by construction or by chance)."""
    t = table.clone()
    t[3, 3] = least
    return bool((t >= least).all())


def stencil64(spec, d, u=None):
    """The definition restated in float64 from the disparity on: (normals (..., h, w, 3) float64 with NaN where invalid, took the flip (bool)).
    Gates, Q and the order of the steps as include/ppms.h has them; nothing is shared with ``OutputSpec.reference``."""
    d = d.double().abs()
    h, w = d.shape[-2:]
    q = spec.Q.double()
    x, y = torch.arange(w, dtype=torch.float64), torch.arange(h, dtype=torch.float64)[:, None]
    v = [q[i, 0] * x + q[i, 1] * y + q[i, 2] * d + q[i, 3] for i in range(4)]
    P = torch.stack([v[i] / v[3] for i in range(3)], dim=-1)
    ok = d >= spec.min_disp
    if spec.max_uncertainty is not None:
        ok = ok & (u.double().abs() <= spec.max_uncertainty)
    if spec.max_depth is not None:
        ok = ok & (P[..., 2] > 0) & (P[..., 2] <= spec.max_depth)

    def shift(t, dy, dx, fill):
        o = torch.full_like(t, fill)
        o[..., max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx), :] = t[..., max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx), :]
        return o

    def side(dy, dx):
        nb, nb_ok = shift(P, dy, dx, 0.0), shift(ok[..., None], dy, dx, False)[..., 0]
        use = ok & nb_ok
        if spec.normal_max_jump is not None:
            use = use & ((nb[..., 2] - P[..., 2]).abs() <= spec.normal_max_jump * P[..., 2].abs())
        return torch.where(use[..., None], nb, P), use

    (r, ur), (l, ul), (dn, ud), (up, uu) = side(0, 1), side(0, -1), side(1, 0), side(-1, 0)
    n = torch.linalg.cross(dn - up, r - l)
    flip = (n * P).sum(-1) > 0
    n = torch.where(flip[..., None], -n, n)
    length = n.norm(dim=-1)
    valid = ok & (ur | ul) & (ud | uu) & (length > 0) & torch.isfinite(length)
    return torch.where(valid[..., None], n / length[..., None], torch.full_like(n, math.nan)), flip


# ---- with a device -------------------------------------------------------------------------------------------------------------------------------
def upsampled(unc, H, W):
    """ppms_bilinear's 4x upsampling of the device tensor unc (T, H/4, W/4): what the kernels compute per pixel, the same bits."""
    return bilinear(unc.view(unc.shape[0], 1, H // 4, W // 4), (H, W), False)


def expected(spec, flow, unc, f0, n, left, top, h0, w0, colour=None):
    """OutputSpec.reference on the host, on the crop of the device state."""
    T, _, H, W = flow.shape
    return spec.reference(crop(flow, f0, n, left, top, h0, w0).cpu(), crop(upsampled(unc, H, W), f0, n, left, top, h0, w0).cpu(), colour)


def launch_normals(spec, plane, flow, unc, f0, n, left, top, h0, w0):
    """ppms_normals_egress with the spec's struct around ``plane`` (an L.EgressPlane)."""
    T, _, H, W = flow.shape
    out = spec.normals_struct({})
    out.normals = plane
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_normals_egress(flow.data_ptr(), unc.data_ptr(), T, H, W, f0, n, left, top, h0, w0, ctypes.byref(out), L.stream_ptr()))
        torch.cuda.synchronize()


def launch_cloud_normals(out, normals, colour, flow, unc, f0, n, left, top, h0, w0):
    """ppms_cloud_egress_normals: ``out`` an L.Cloud, ``normals`` / ``colour`` L.EgressPlane (colour: None = NULL)."""
    T, _, H, W = flow.shape
    with torch.cuda.device(DEV):
        L.check(L.load().ppms_cloud_egress_normals(flow.data_ptr(), unc.data_ptr(), T, H, W, f0, n, left, top, h0, w0, ctypes.byref(out), ctypes.byref(normals),
                                                   None if colour is None else ctypes.byref(colour), L.stream_ptr()))
        torch.cuda.synchronize()
