"""Plain float64 CPU references of the non-convolution kernels of the two encoders (encoder_ops.hip), of the glue kernels around the
loop (glue_ops.hip, loop_ops.hip), of the kernels inside every update iteration (corr.hip's lookup, pwchain.hip, ppms_dwconv_gelu, attn16.hip), of
the pick-and-play memory read-out (frame similarity, QAM pick, attention operands, mem_attn.hip) and of the correlation build and the flow
output kernels (corr.hip's pyramid build, convex upsampling 2-D / 3-D, tap gather-sum, bilinear resize, the four tiled transposes), one
function per operation, each with the named wrong variants its test exists to catch; the cases (shapes and seeded inputs) of
tests/test_gpu_encoder_ops.py, tests/test_gpu_glue_ops.py, tests/test_gpu_update_ops.py, tests/test_gpu_memory_ops.py and
tests/test_gpu_flow_ops.py; and the tolerance rule they and the CPU test tests/test_kernel_refs.py apply.  The formulas are those of
oracle/ppm_oracle.py and of the kernel comments.

Tolerances, three kinds, none taken from the code under test:
 (a) exact: copies, permutations (the tiled transposes), the relu half, flow_add, the accum side of the tap gather-sum, the hi plane of
     any split (Check.exact);
 (b) split-bf16 outputs of elementwise math: 2e-5 * max(1, max|ref|), the bound the suite uses for that storage (tol_sp);
 (c) reductions and transcendentals: 8 x the max error of the same operation in plain fp32 torch on the CPU, on the same input, against
     the float64 reference -- or (b) where the output is split bf16, whichever is larger (tol_reduce).  8: the kernels sum in a fixed
     order of their own (per thread over its pixels, a butterfly over the rows of a wave, the waves, then the slices) where torch sums
     in cascades; that costs a small factor, not an order.
"""
import functools
import math

import torch
import torch.nn.functional as F

from ppmstereo_amd.weights import hash_normal

F64 = torch.float64
SENTINEL = 1.0                                                            # what every output buffer holds before a launch
JUNK = 777.0                                                              # what padding columns of fp32 inputs hold: never to be read


# ------------------------------------------------------------------------------------------------ split bf16, tolerances
def sp_split(x: torch.Tensor):
    """(hi, lo) bf16 planes of fp32 x as every kernel stores them: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def sp_round(x: torch.Tensor) -> torch.Tensor:
    """fp32 value a split-bf16 pair holds for x (what SPTensor.set_f32 followed by to_f32 gives)."""
    hi, lo = sp_split(x)
    return hi.float() + lo.float()


def tol_sp(ref: torch.Tensor) -> float:
    return 2e-5 * max(1.0, ref.abs().max().item())


def tol_reduce(ref: torch.Tensor, f32: torch.Tensor, split: bool) -> float:
    t = 8.0 * (f32.double() - ref.double()).abs().max().item()
    return max(t, tol_sp(ref)) if split else t


class Check:
    """The outcome of comparing one case: (name, error, tolerance) items.  A shape mismatch is an infinite error."""

    def __init__(self, label=""):
        self.label, self.items = label, []

    def add(self, name, got, ref, tol):
        got, ref = got.detach().cpu().double(), ref.double()
        if got.shape != ref.shape or not torch.isfinite(got).all():
            self.items.append((name, math.inf, float(tol)))
        else:
            self.items.append((name, (got - ref).abs().max().item() if ref.numel() else 0.0, float(tol)))
        return self

    def bound(self, name, got, ref, tol_each):
        """elementwise bound: error = max(|got - ref| - tol_each) must be <= 0"""
        got, ref = got.detach().cpu().double(), ref.double()
        if got.shape != ref.shape or not torch.isfinite(got).all():
            self.items.append((name, math.inf, 0.0))
        else:
            self.items.append((name, ((got - ref).abs() - tol_each.double()).max().item(), 0.0))
        return self

    def exact(self, name, got, ref):
        got = got.detach().cpu()
        bad = math.inf if got.shape != ref.shape else float((got != ref).sum().item())
        self.items.append((name, bad, 0.0))
        return self

    @property
    def ok(self):
        return all(e <= t for _, e, t in self.items)

    def worst(self):
        """largest error / tolerance over the items with a tolerance"""
        return max([e / t for _, e, t in self.items if t > 0.0] or [0.0])

    def __str__(self):
        return self.label + ": " + ", ".join(f"{n} {e:.3e}/{t:.3e}" for n, e, t in self.items)


# ------------------------------------------------------------------------------------------------ InstanceNorm
IN_EPS = 1e-5
INSTNORM_CASES = {  # N, C, HW, ld, channels of the out view, x one float into its allocation
    "A": (1, 64, 4225, 64, 72, False),        # S = 66 slices of 65 pixels: slice 65 is empty, the merge's 8-wide groups end in a tail of 2
    "B": (2, 96, 35, 96, 104, False),         # S = 1; rows 0-2 carry two pixels each, the rest one
    "C": (3, 40, 700, 44, 48, False),         # last channel block 8 wide, ld != C, S = 10
    "D": (1, 30, 130, 31, 32, True),          # scalar paths of part and apply (ld % 4 != 0, C % 8 != 0, base not 16-B aligned); out channels 30, 31 zero
}


def in_slices(N, HW, C):
    """pixel slices of the instnorm / GRN part kernels: (S, chunk), re-derived from in_slices_host"""
    S = max(1, min(1024 // (((C + 31) // 32) * N), HW // 64))
    return S, (HW + S - 1) // S


def _in_apply(x, mean, rstd, res, relu):
    y = (x.double() - mean[:, None]) * rstd[:, None]
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0.0) if relu else y


def instnorm(x, eps, res=None, relu=False):
    """x (N, HW, C), res (N, HW, C) or None -> mean (N, C), rstd (N, C), y (N, HW, C): biased variance over the pixels"""
    x = x.double()
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    return mean, rstd, _in_apply(x, mean, rstd, res, relu)


def instnorm_f32(x, eps, res=None, relu=False):
    """the same in plain fp32 torch (tolerance kind c)"""
    x = x.float()
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + eps).rsqrt()
    y = F.instance_norm(x.permute(0, 2, 1), eps=eps).permute(0, 2, 1)
    if res is not None:
        y = y + res.float()
    return mean, rstd, (y.clamp_min(0.0) if relu else y)


def _in_unbiased(x, eps, res=None, relu=False):
    x = x.double()
    mean, rstd = x.mean(1), (x.var(1, unbiased=True) + eps).rsqrt()
    return mean, rstd, _in_apply(x, mean, rstd, res, relu)


def _in_eps6(x, eps, res=None, relu=False):
    return instnorm(x, 1e-6, res, relu)


def _in_one_pass(x, eps, res=None, relu=False):
    x32 = x.float()
    m = x32.mean(1)
    var = ((x32 * x32).mean(1) - m * m).clamp_min(0.0)                    # E[x^2] - E[x]^2 in fp32
    mean, rstd = m.double(), (var.double() + eps).rsqrt()
    return mean, rstd, _in_apply(x, mean, rstd, res, relu)


def _in_last_slice_dropped(x, eps, res=None, relu=False):
    """the merge stops one (non-empty) slice early: mean over the pixels it saw, M2 / HW.  None where there is one slice only."""
    N, HW, C = x.shape
    S, chunk = in_slices(N, HW, C)
    keep = ((HW + chunk - 1) // chunk - 1) * chunk
    if keep <= 0:
        return None
    xk = x.double()[:, :keep]
    mean = xk.mean(1)
    rstd = (((xk - mean[:, None]) ** 2).sum(1) / HW + eps).rsqrt()
    return mean, rstd, _in_apply(x, mean, rstd, res, relu)


INSTNORM_WRONG = {"unbiased": _in_unbiased, "eps_1e-6": _in_eps6, "one_pass_fp32": _in_one_pass, "last_slice_dropped": _in_last_slice_dropped}


@functools.lru_cache(maxsize=None)
def instnorm_inputs(case, data):
    """x (N, HW, C) fp32: data "unit" = hash_normal, "offset" = 50 + 0.05 hash_normal; res (N, HW, roundup8(C)) as split bf16 holds it"""
    N, C, HW, ld, outc, misaligned = INSTNORM_CASES[case]
    seed = 7000 + 10 * "ABCD".index(case)
    x = hash_normal((N, HW, C), seed)
    if data == "offset":
        x = (50.0 + 0.05 * x).float()
    res = sp_round(hash_normal((N, HW, (C + 7) // 8 * 8), seed + 1))
    return x, res


def instnorm_check(case, data, with_res, relu, mean, rstd, y, label=None):
    x, res = instnorm_inputs(case, data)
    C = x.shape[2]
    r = res[:, :, :C] if with_res else None
    ref, f32 = instnorm(x, IN_EPS, r, relu), instnorm_f32(x, IN_EPS, r, relu)
    ck = Check(label or f"instnorm {case} {data} res={int(with_res)} relu={int(relu)}")
    ck.add("mean", mean, ref[0], tol_reduce(ref[0], f32[0], False))
    ck.add("rstd", rstd, ref[1], tol_reduce(ref[1], f32[1], False))
    return ck.add("y", y, ref[2], tol_reduce(ref[2], f32[2], True))


# ------------------------------------------------------------------------------------------------ GRN
GRN_CASES = {  # N, HW, C, ld, input scale
    "small": (2, 35, 96, 96, 1.0),
    "empty_slice": (1, 4225, 64, 64, 1.0),    # S = 66, chunk 65: slice 65 is empty
    "wide": (1, 130, 3072, 3072, 1.0),        # the merge's loop over C > 256, S = 2
    "tiny": (1, 35, 96, 104, 2e-6),           # |x| ~ 2e-6, gamma scaled by 1 / max|x|: the 1e-6 of the divisor matters
    "scalar": (1, 35, 96, 97, 1.0),           # ld % 4 != 0: the scalar paths of grn_part and grn_apply
}


def _grn_from(h, gx, eps, gamma, beta):
    nx = gx / (gx.mean(dim=-1, keepdim=True) + eps)
    return gamma.double() * (h * nx) + beta.double() + h


def grn(h, gamma, beta):
    """h (N, HW, C): Gx = ||h||_2 over the pixels, Nx = Gx / (mean_c Gx + 1e-6), gamma (h Nx) + beta + h"""
    h = h.double()
    return _grn_from(h, torch.norm(h, p=2, dim=1, keepdim=True), 1e-6, gamma, beta)


def grn_f32(h, gamma, beta):
    h = h.float()
    gx = torch.norm(h, p=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    return gamma.float() * (h * nx) + beta.float() + h


def _grn_eps5(h, gamma, beta):
    h = h.double()
    return _grn_from(h, torch.norm(h, p=2, dim=1, keepdim=True), 1e-5, gamma, beta)


def _grn_mean_over_pixels(h, gamma, beta):
    """the two axes swapped: the norm over the channels of a pixel, its mean over the pixels"""
    h = h.double()
    gx = torch.norm(h, p=2, dim=2, keepdim=True)
    return gamma.double() * (h * (gx / (gx.mean(dim=1, keepdim=True) + 1e-6))) + beta.double() + h


def _grn_no_sqrt(h, gamma, beta):
    h = h.double()
    return _grn_from(h, (h * h).sum(1, keepdim=True), 1e-6, gamma, beta)


GRN_WRONG = {"eps_1e-5": _grn_eps5, "mean_over_pixels": _grn_mean_over_pixels, "no_sqrt": _grn_no_sqrt}


@functools.lru_cache(maxsize=None)
def grn_inputs(case):
    N, HW, C, ld, scale = GRN_CASES[case]
    seed = 7100 + 10 * list(GRN_CASES).index(case)
    h = (hash_normal((N, HW, C), seed) * scale).float()
    gamma = (hash_normal((C,), seed + 1) / (h.abs().max().item() if scale != 1.0 else 1.0)).float()
    return h, gamma, hash_normal((C,), seed + 2) * 0.1


def grn_check(case, y):
    h, gamma, beta = grn_inputs(case)
    ref = grn(h, gamma, beta)
    return Check(f"grn {case}").add("y", y, ref, tol_reduce(ref, grn_f32(h, gamma, beta), True))


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-6
LN_PIXELS = 37                                                             # not a multiple of the 4 pixels of a workgroup
LN_CASES = {96: 96, 520: 520, 768: 768, 1024: 1024, 36: 40}                # C -> channels of the out view (520: second round with one active
#                                                                            lane; 1024: the limit; 36: scalar path, channels 36-39 zero)


def layernorm(x, w, b, eps):
    """x (P, C): per pixel over C, biased variance, affine"""
    x = x.double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    return (x - mean) * (var + eps).rsqrt() * w.double() + b.double()


def layernorm_f32(x, w, b, eps):
    return F.layer_norm(x.float(), (x.shape[1],), w.float(), b.float(), eps)


def _ln_eps5(x, w, b, eps):
    return layernorm(x, w, b, 1e-5)


def _ln_unbiased(x, w, b, eps):
    x = x.double()
    return (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=True, keepdim=True) + eps).rsqrt() * w.double() + b.double()


LN_WRONG = {"eps_1e-5": _ln_eps5, "unbiased": _ln_unbiased}


@functools.lru_cache(maxsize=None)
def layernorm_inputs(C):
    """every third row scaled by 1e-2 (eps matters), every third row plus one is 20 + 0.3 x (cancellation), the rest unit"""
    x = hash_normal((LN_PIXELS, C), 7200 + C)
    x[0::3] *= 1e-2
    x[1::3] = 20.0 + 0.3 * x[1::3]
    return x, 1.0 + 0.1 * hash_normal((C,), 7201 + C), 0.1 * hash_normal((C,), 7202 + C)


def layernorm_check(C, y):
    x, w, b = layernorm_inputs(C)
    ref = layernorm(x, w, b, LN_EPS)
    return Check(f"layernorm C={C}").add("y", y, ref, tol_reduce(ref, layernorm_f32(x, w, b, LN_EPS), True))


# ------------------------------------------------------------------------------------------------ depthwise 7 x 7
DW_CASES = [(2, 1, 2, 96), (1, 5, 7, 192), (1, 4, 9, 768), (2, 8, 16, 64)]   # N, H, W, C: a last block of 32 channels with W < 4; W % 4 != 0


def _dw_taps(x, w, b, pad_mode, flip):
    """x (N, H, W, C), w (C, 49), b (C,) -> (N, H, W, C) float64, tap by tap"""
    N, H, W, C = x.shape
    xp = x.double().permute(0, 3, 1, 2)
    xp = F.pad(xp, (3, 3, 3, 3)) if pad_mode == "zeros" else xp[:, :, torch.arange(-3, H + 3).clamp(0, H - 1)][:, :, :, torch.arange(-3, W + 3).clamp(0, W - 1)]
    w = w.double().reshape(C, 7, 7)
    if flip:
        w = w.flip(1, 2)
    y = b.double().reshape(1, C, 1, 1).expand(N, C, H, W).clone()
    for ky in range(7):
        for kx in range(7):
            y += xp[:, :, ky:ky + H, kx:kx + W] * w[:, ky, kx].reshape(1, C, 1, 1)
    return y.permute(0, 2, 3, 1)


def dwconv(x, w, b):
    """depthwise 7 x 7 cross-correlation plus bias, zero padding"""
    return _dw_taps(x, w, b, "zeros", False)


def dwconv_f32(x, w, b):
    C = x.shape[3]
    return F.conv2d(x.float().permute(0, 3, 1, 2), w.float().reshape(C, 1, 7, 7), b.float(), padding=3, groups=C).permute(0, 2, 3, 1)


DW_WRONG = {"flipped": lambda x, w, b: _dw_taps(x, w, b, "zeros", True), "clamped": lambda x, w, b: _dw_taps(x, w, b, "clamp", False)}


@functools.lru_cache(maxsize=None)
def dwconv_inputs(case):
    N, H, W, C = case
    seed = 7300 + C + W
    return sp_round(hash_normal((N, H, W, C), seed)), hash_normal((C, 49), seed + 1) / 7.0, hash_normal((C,), seed + 2) * 0.1


def dwconv_check(case, y):
    x, w, b = dwconv_inputs(case)
    ref = dwconv(x, w, b)
    return Check(f"dwconv {case}").add("y", y, ref, tol_reduce(ref, dwconv_f32(x, w, b), False))


# ------------------------------------------------------------------------------------------------ layout: space to depth, upsample
def s2d(x, k, swap=False):
    """x (N, H, W, C) -> (N, H / k, W / k, k k C): out[n, i, j, phase C + c] = x[n, k i + dy, k j + dx, c], phase = k dy + dx"""
    N, H, W, C = x.shape
    v = x.reshape(N, H // k, k, W // k, k, C)                              # n, i, dy, j, dx, c
    v = v.permute(0, 1, 3, 4, 2, 5) if swap else v.permute(0, 1, 3, 2, 4, 5)
    return v.reshape(N, H // k, W // k, k * k * C)


S2D_WRONG = {"dy_dx_swapped": lambda x, k: s2d(x, k, swap=True)}


def upsample2(x):
    """nearest x2: out[n, y, x] = in[n, y >> 1, x >> 1]"""
    N, H, W, C = x.shape
    return x[:, torch.arange(2 * H) >> 1][:, :, torch.arange(2 * W) >> 1]


def _upsample2_round_up(x):
    N, H, W, C = x.shape
    return x[:, ((torch.arange(2 * H) + 1) >> 1).clamp_max(H - 1)][:, :, ((torch.arange(2 * W) + 1) >> 1).clamp_max(W - 1)]


UP_WRONG = {"(y+1)>>1": _upsample2_round_up}


# ------------------------------------------------------------------------------------------------ flow patch (7 x 7 im2col)
def flow_patch(flow, order="ky_major"):
    """flow (BT, H, W, 2) -> (BT, H, W, 128): column tap 2 + c, tap = ky 7 + kx, of the zero-padded 7 x 7 window; columns 98-127 zero"""
    BT, H, W, _ = flow.shape
    fp = F.pad(flow.permute(0, 3, 1, 2), (3, 3, 3, 3)).permute(0, 2, 3, 1)
    out = torch.zeros(BT, H, W, 128, dtype=flow.dtype)
    for ky in range(7):
        for kx in range(7):
            tap = ky * 7 + kx if order == "ky_major" else kx * 7 + ky
            out[..., 2 * tap:2 * tap + 2] = fp[:, ky:ky + H, kx:kx + W]
    return out


PATCH_WRONG = {"tap=kx*7+ky": lambda flow: flow_patch(flow, "kx_major")}


# ------------------------------------------------------------------------------------------------ resize-blend, avgpool, axpby, ctx_mix, unc tail
def resize_blend(dst, src, OH, OW, a, b):
    """dst (N, OH, OW, C), src (N, H, W, C): a dst + b interp(src), bilinear, align_corners=True (a = 0: dst is not read)"""
    N, H, W, C = src.shape
    s = src.double()
    fy = torch.arange(OH, dtype=F64) * ((H - 1) / (OH - 1) if OH > 1 else 0.0)
    fx = torch.arange(OW, dtype=F64) * ((W - 1) / (OW - 1) if OW > 1 else 0.0)
    y0, x0 = fy.floor().long().clamp(0, H - 1), fx.floor().long().clamp(0, W - 1)
    y1, x1 = (y0 + 1).clamp_max(H - 1), (x0 + 1).clamp_max(W - 1)
    ly, lx = (fy - y0).reshape(1, OH, 1, 1), (fx - x0).reshape(1, 1, OW, 1)
    rows = lambda yy: s[:, yy][:, :, x0] * (1 - lx) + s[:, yy][:, :, x1] * lx
    v = rows(y0) * (1 - ly) + rows(y1) * ly
    return b * v if a == 0.0 else a * dst.double() + b * v


def _resize_half_pixel(dst, src, OH, OW, a, b):
    v = F.interpolate(src.double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    return b * v if a == 0.0 else a * dst.double() + b * v


RESIZE_WRONG = {"align_corners=False": _resize_half_pixel}


def avgpool(x, k):
    """x (planes, H, W): windows of k x k at stride k, output sizes floored"""
    P, H, W = x.shape
    OH, OW = H // k, W // k
    return x.double()[:, :OH * k, :OW * k].reshape(P, OH, k, OW, k).mean((2, 4))


def avgpool_f32(x, k):
    return F.avg_pool2d(x.float()[None], k, stride=k)[0]


def _avgpool_clipped(x, k):
    """pools the ragged border too: ceil sizes, the divisor counts the pixels of the window that lie inside the image.  With floored
    output sizes no window is ever clipped, so on the floored region this variant gives the reference's values: what catches it is the
    size of its output (9 x 14 at k = 4 -> 3 x 4 instead of 2 x 3).  The case guards the floor of the output sizes."""
    return F.avg_pool2d(x.double()[None], k, stride=k, ceil_mode=True, count_include_pad=False)[0]


AVGPOOL_WRONG = {"clipped_divisor": _avgpool_clipped}


def axpby(x, y, a, b, period):
    """a x[i] + b y[i mod period] on flat arrays"""
    n = x.numel()
    return a * x.double().reshape(-1) + b * y.double().reshape(-1)[torch.arange(n) % period]


def axpby_tol(x, y, a, b, period):
    """per element: two products and a sum in fp32, fused or not -- three roundings of at most 2^-24 relative to |a x| + |b y|"""
    n = x.numel()
    return 3 * 2.0 ** -24 * ((a * x.double().reshape(-1)).abs() + (b * y.double().reshape(-1)[torch.arange(n) % period]).abs())


def ctx_mix(f, c):
    """f, c (N, 256, HW) -> net = tanh of the mean of the first 128 channels, inp = relu of the mean of the last 128"""
    m = (f.double() + c.double()) / 2
    return torch.tanh(m[:, :128]), m[:, 128:].clamp_min(0.0)


def ctx_mix_f32(f, c):
    m = (f.float() + c.float()) / 2.0
    return torch.tanh(m[:, :128]), m[:, 128:].clamp_min(0.0)


def unc_tail(x, w, bias):
    """x (BT, HW, 128): unc = sigmoid(w . x + bias) (BT, HW); partial (BT, ceil(HW / 256)) = its sums over blocks of 256 pixels"""
    BT, HW, _ = x.shape
    unc = torch.sigmoid(x.double() @ w.double() + bias)
    nblk = (HW + 255) // 256
    return unc, F.pad(unc, (0, nblk * 256 - HW)).reshape(BT, nblk, 256).sum(2)


def unc_tail_f32(x, w, bias):
    return torch.sigmoid(x.float() @ w.float() + bias)


def unc_partial_tol(tol_unc):
    """256 x the unc tolerance plus 255 2^-24 256: the worst case of any-order fp32 summation of 256 terms <= 1"""
    return 256.0 * tol_unc + 255.0 * 2.0 ** -24 * 256.0


# ------------------------------------------------------------------------------------------------ cases and inputs of the layout / glue kernels
UP_CASE = (2, 3, 5)                                                        # N, H, W
S2D_CASES = [(2, 6, 10, 8), (2, 6, 10, 96)]                                # N, H, W, C
IMG_S2D_CASES = [(2, (2, 3, 6, 10), 16), (4, (2, 3, 8, 12), 48), (4, (2, 3, 8, 12), 64)]      # k, image shape, channels of the dst view
PATCH_CASES = [(2, 5, 9), (1, 3, 3)]                                       # BT, H, W: windows cross both borders at once
UNC_CASES = [(2, 700), (3, 5), (1, 256)]                                   # BT, HW
RESIZE_CASES = [(2, 3, 5, 6, 10), (1, 1, 4, 2, 8), (1, 4, 4, 4, 4)]        # N, H, W, OH, OW
RESIZE_AB = [(0.0, 1.0), (0.5, 0.5)]
AVGPOOL_CASES = [(4, 8, 12), (2, 8, 12), (4, 9, 14)]                       # k, H, W on 6 planes
AXPBY_CASES = [(1000, 1000, 0.5, 0.5), (1000, 250, 1.0, 1.0)]              # n, period, a, b


def upsample_input():
    """the 32 channels of the source tensor of the sp_upsample2 case (the view is channels 8-23)"""
    N, H, W = UP_CASE
    return sp_values((N * H * W, 32), 7900)


def s2d_input(case):
    N, H, W, C = case
    return sp_values((N * H * W, C), 7910 + C)


def sp_values(shape, seed):
    """fp32 values that a split-bf16 tensor holds exactly"""
    return sp_round(hash_normal(shape, seed))


def img_input(shape):
    return hash_normal(shape, 7400 + shape[2])


def flow_input(case):
    BT, H, W = case
    return hash_normal((BT, H, W, 2), 7500 + H) * 3.0


def unc_inputs(case):
    BT, HW = case
    return sp_values((BT, HW, 128), 7600 + HW), hash_normal((128,), 7601) * (2.0 / math.sqrt(128.0)), 0.3


def resize_inputs(case):
    """(dst, src) values of the 16 channels of the views"""
    N, H, W, OH, OW = case
    return sp_values((N, OH, OW, 16), 7700 + OW), sp_values((N, H, W, 16), 7701 + OW)


def avgpool_input(case):
    k, H, W = case
    return hash_normal((6, H, W), 7800 + 10 * k + H)


def split_check(ck, name, hi, lo, ref):
    """the split of fp32 `ref` into planes: hi is bf16(ref) exactly; each of the two roundings to 8 significant bits costs at most 2^-8
    relative, so |hi + lo - ref| <= 2^-16 |ref|"""
    ck.exact(name + ".hi", hi, ref.to(torch.bfloat16))
    return ck.bound(name + ".hi+lo", hi.float().double() + lo.float().double(), ref, ref.double().abs() * 2.0 ** -16)


# ================================================================================================ kernels of the update iteration
# The correlation lookup (corr.hip), the correlation encoder (pwchain.hip, ppms_dwconv_gelu) and the block16 / SST attention helpers
# (attn16.hip): tests/test_gpu_update_ops.py.  Same three tolerance kinds; the pwchain cases keep the bounds the suite already uses for
# that kernel (PW_ACC for one layer -- conv_audit.ACC_MAX --, 3e-5 / 5e-5 for the engine's chains), now against float64.
def _gelu(v, form="erf"):
    return F.gelu(v, approximate="tanh" if form == "tanh" else "none")


# ------------------------------------------------------------------------------------------------ correlation lookup
LOOKUP_CASES = {  # B, H, W
    "P54": (1, 3, 18),                         # P % 4 = 2, W % 4 != 0, widths 18 / 9 / 4 / 2
    "W16": (2, 2, 16),                         # the narrowest map the entry point accepts: level 3 has two columns
    "W40": (1, 1, 40),                         # widths 40 / 20 / 10 / 5
}


def corr_lookup(levels, flow_x, W, tap_shift=0, scaled=True, half_pixel=False, clamp=False):
    """levels: 4 pyramid levels (P, W >> l); flow_x (P,) -> (P, 36) float64, channel 9 l + kk: linear interpolation of the pixel's row of
    level l at p = (kk - 4) + (x + flow_x) / 2^l, taps outside [0, Wl - 1] contribute 0 (corr.py:74-94: grid_sample, align_corners=True,
    zero padding).  The keyword arguments are the wrong variants."""
    P = flow_x.shape[0]
    xs = (torch.arange(P) % W).double() + flow_x.double()
    outs = []
    for l, L in enumerate(levels):
        L, Wl = L.double(), L.shape[1]
        p = (torch.arange(9, dtype=F64) - 4 + tap_shift)[None] + xs[:, None] / (2 ** l if scaled else 1)
        if half_pixel:
            p = p * Wl / (Wl - 1) - 0.5                                   # g = 2 p / (Wl - 1) - 1 un-normalised as ((g + 1) Wl - 1) / 2
        if clamp:
            p = p.clamp(0, Wl - 1)
        p0 = p.floor()
        a, i0 = p - p0, p0.long()
        tap = lambda i: torch.gather(L, 1, i.clamp(0, Wl - 1)) * ((i >= 0) & (i <= Wl - 1))
        outs.append((1 - a) * tap(i0) + a * tap(i0 + 1))
    return torch.cat(outs, 1)


def corr_lookup_f32(levels, flow, B, H, W):
    """the oracle's fp32 op sequence (normalise, un-normalise as the reference does): flow (P, 2) -> (P, 36)"""
    from oracle import ppm_oracle as O
    out = O.corr_lookup([L.float() for L in levels], flow.float().reshape(B, H, W, 2).permute(0, 3, 1, 2))
    return out.permute(0, 2, 3, 1).reshape(B * H * W, 36)


LOOKUP_WRONG = {
    "tap_shifted": lambda lv, fx, W: corr_lookup(lv, fx, W, tap_shift=1),
    "no_level_scale": lambda lv, fx, W: corr_lookup(lv, fx, W, scaled=False),
    "half_pixel": lambda lv, fx, W: corr_lookup(lv, fx, W, half_pixel=True),
    "border_clamp": lambda lv, fx, W: corr_lookup(lv, fx, W, clamp=True),
}


@functools.lru_cache(maxsize=None)
def lookup_inputs(case):
    """levels: 4 x (P, W >> l) fp32; flow (P, 2) fp32 = 3 hash_normal, every 5th column rounded to an integer (a = 0), every 7th column x 8
    (out of range); then pixels 1-8: the outermost tap of level l lands exactly on column Wl - 1 (pixel 1 + 2 l: tap kk = 0) and on column 0
    (pixel 2 + 2 l: tap kk = 8); pixels 9, 10: +1e9, -1e9"""
    B, H, W = LOOKUP_CASES[case]
    P, seed = B * H * W, 8000 + 10 * list(LOOKUP_CASES).index(case)
    levels = tuple(hash_normal((P, W >> l), seed + l) for l in range(4))
    flow = 3.0 * hash_normal((P, 2), seed + 5)
    x = torch.arange(P) % W
    flow[x % 5 == 0] = flow[x % 5 == 0].round()
    flow[x % 7 == 0] *= 8.0
    for l in range(4):
        Wl = W >> l
        flow[1 + 2 * l, 0] = float(2 ** l * (Wl - 1 + 4) - x[1 + 2 * l])      # (x + fx) / 2^l - 4 = Wl - 1
        flow[2 + 2 * l, 0] = float(-4 * 2 ** l - x[2 + 2 * l])                # (x + fx) / 2^l + 4 = 0
    flow[9, 0], flow[10, 0] = 1e9, -1e9
    return levels, flow


@functools.lru_cache(maxsize=None)
def lookup_refs(case):
    B, H, W = LOOKUP_CASES[case]
    levels, flow = lookup_inputs(case)
    return corr_lookup(levels, flow[:, 0], W), corr_lookup_f32(levels, flow, B, H, W)


def lookup_check(case, got, split, label=None):
    """got (P, 36)"""
    ref, f32 = lookup_refs(case)
    return Check(label or f"corr_lookup {case}").add("corr", got, ref, tol_reduce(ref, f32, split))


# ------------------------------------------------------------------------------------------------ depthwise k x k + residual GELU
DWG_CASES = {  # BT, H, W, channels of the view, ld, k
    "edges": (2, 3, 5, 8, 16, 7),              # every window crosses the top and bottom of its frame and both row ends; the last run of a row holds one pixel
    "view40": (1, 9, 17, 40, 64, 7),           # the engine's view: channels 40-63 of x hold junk, those of y keep the sentinel
    "full64": (3, 8, 16, 64, 72, 7),
    "view40_k1": (1, 9, 17, 40, 64, 1),
}


def dwconv_gelu(x, w, b, k, pad="zeros", flip=False, transpose=False, residual=True, bias=True, gelu="erf", frames=True):
    """x (BT, H, W, C), w (C, k k), b (C,) -> gelu_erf(x + dw_k(x) + b) (BT, H, W, C) float64, tap by tap: cross-correlation, zero padding
    inside each frame (ppmtereo_update.py:1026-1027).  The keyword arguments are the wrong variants."""
    BT, H, W, C = x.shape
    if not frames:                                                          # taps read the neighbouring frame: one frame of BT H rows
        return dwconv_gelu(x.reshape(1, BT * H, W, C), w, b, k, pad, flip, transpose, residual, bias, gelu).reshape(BT, H, W, C)
    R, P = k // 2, BT * H * W
    xd, wd = x.double(), w.double().reshape(C, k, k)
    if flip:
        wd = wd.flip(1, 2)
    if transpose:
        wd = wd.transpose(1, 2)
    flat = xd.reshape(P, C)
    f, y, xx0 = torch.arange(BT).reshape(BT, 1, 1), torch.arange(H).reshape(1, H, 1), torch.arange(W).reshape(1, 1, W)
    acc = torch.zeros(BT, H, W, C, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            yy, xx = y + ky - R, xx0 + kx - R
            if pad == "replicate":
                yy, xx = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
            q = ((f * H + yy) * W + xx).expand(BT, H, W)
            if pad == "zeros":
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            elif pad == "y_only":                                           # no test along x: the tap wraps into the neighbouring row
                ok = (yy >= 0) & (yy < H) & (q >= 0) & (q < P)
            else:
                ok = torch.ones(1, 1, 1, dtype=torch.bool)
            v = flat[q.clamp(0, P - 1).reshape(-1)].reshape(BT, H, W, C) * ok.expand(BT, H, W)[..., None]
            acc += v * wd[:, ky, kx]
    v = acc + (b.double() if bias else 0.0) + (xd if residual else 0.0)
    return _gelu(v, gelu)


def dwconv_gelu_f32(x, w, b, k):
    C = x.shape[3]
    xi = x.float().permute(0, 3, 1, 2)
    return F.gelu(xi + F.conv2d(xi, w.float().reshape(C, 1, k, k), b.float(), padding=k // 2, groups=C)).permute(0, 2, 3, 1)


DWG_WRONG = {
    "flipped": dict(flip=True), "ky_kx_transposed": dict(transpose=True), "no_residual": dict(residual=False), "no_bias": dict(bias=False),
    "tanh_gelu": dict(gelu="tanh"), "replicate_padding": dict(pad="replicate"), "zero_padding_in_y_only": dict(pad="y_only"),
    "no_frame_boundary": dict(frames=False),
}


@functools.lru_cache(maxsize=None)
def dwg_inputs(case):
    BT, H, W, c, ld, k = DWG_CASES[case]
    seed = 8100 + 10 * list(DWG_CASES).index(case)
    return sp_round(hash_normal((BT, H, W, c), seed)), hash_normal((c, k * k), seed + 1) / k, hash_normal((c,), seed + 2) * 0.1


@functools.lru_cache(maxsize=None)
def dwg_refs(case):
    x, w, b = dwg_inputs(case)
    k = DWG_CASES[case][5]
    return dwconv_gelu(x, w, b, k), dwconv_gelu_f32(x, w, b, k)


def dwg_check(case, y):
    ref, f32 = dwg_refs(case)
    return Check(f"dwconv_gelu {case}").add("y", y, ref, tol_reduce(ref, f32, True))


# ------------------------------------------------------------------------------------------------ fused per-pixel chains
PW_ACC = 3e-5                                                              # conv_audit.ACC_MAX, the project's bound for one conv layer
PW_PIXELS = [1, 318, 16384, 16385]                                         # 16384: the last count of the 32-pixel-tile kernel; 16385: the 128-pixel
#                                                                            kernel, whose last tile holds one pixel
PW_CHAINS = {  # input channels, [(cout, cin, residual, post affine)], bound relative to max(1, max|ref|)
    "s64": (64, [(64, 64, False, False)], PW_ACC),
    "s64_res": (64, [(64, 64, True, False)], PW_ACC),
    "s64_post": (64, [(64, 64, False, True)], PW_ACC),
    "s64_res_post": (64, [(64, 64, True, True)], PW_ACC),
    "s256": (64, [(256, 64, False, False)], PW_ACC),
    "A": (36, [(54, 36, False, False), (36, 54, True, True)], 3e-5),                                  # ffn1 + the depthwise 1x1 (engine.py chainA)
    "B": (36, [(36, 36, True, False), (54, 36, False, False), (256, 54, False, False)], 5e-5),         # pw + ffn2 + the outer gelu (chainB)
}


def pwchain(x, layers, gelu="erf", resid_from="input", post_first=False, bias=True):
    """x (P, cin); layers: [(w (cout, cin), b (cout,), residual, (s, t) or None)] -> (P, cout of the last layer) float64.  Per layer
    y = gelu(w v + b [+ the chain INPUT at the same channel]); with a post step y = gelu(y + (y s + t)) (pwchain.hip).  The keyword
    arguments are the wrong variants."""
    x0 = x.double()
    v = x0
    for w, b, resid, post in layers:
        co = w.shape[0]
        y = v[:, :w.shape[1]] @ w.double().t() + (b.double() if bias else 0.0)
        if resid:
            y = y + (x0 if resid_from == "input" else v)[:, :co]
        if post is not None and post_first:
            y = y + (y * post[0].double() + post[1].double())
            v = _gelu(_gelu(y, gelu), gelu)
            continue
        y = _gelu(y, gelu)
        if post is not None:
            y = _gelu(y + (y * post[0].double() + post[1].double()), gelu)
        v = y
    return v


def pwchain_f32(x, layers):
    x0 = x.float()
    v = x0
    for w, b, resid, post in layers:
        y = v[:, :w.shape[1]] @ w.float().t() + b.float()
        if resid:
            y = y + x0[:, :w.shape[0]]
        y = F.gelu(y)
        v = F.gelu(y + (y * post[0].float() + post[1].float())) if post is not None else y
    return v


PW_WRONG = {"tanh_gelu": dict(gelu="tanh"), "residual_from_previous_layer": dict(resid_from="previous"),
            "post_before_activation": dict(post_first=True), "no_bias": dict(bias=False)}


@functools.lru_cache(maxsize=None)
def pwchain_layers(chain):
    """weights as the packs hold them (split bf16), fp32 bias and post affine"""
    cin, spec, _ = PW_CHAINS[chain]
    seed = 8200 + 20 * list(PW_CHAINS).index(chain)
    layers = []
    for i, (co, ci, resid, post) in enumerate(spec):
        w = sp_round(hash_normal((co, ci), seed + 4 * i) / math.sqrt(ci))
        st = (hash_normal((co,), seed + 4 * i + 2) * 0.5, hash_normal((co,), seed + 4 * i + 3) * 0.1) if post else None
        layers.append((w, hash_normal((co,), seed + 4 * i + 1) * 0.1, resid, st))
    return tuple(layers)


@functools.lru_cache(maxsize=None)
def pwchain_input():
    """(max P, 64): every case reads its first P rows and its first cin channels"""
    return sp_round(hash_normal((max(PW_PIXELS), 64), 8190))


@functools.lru_cache(maxsize=None)
def pwchain_ref(chain):
    """the reference of all max(PW_PIXELS) rows (the operation is per pixel: a case of P pixels compares with the first P rows)"""
    cin = PW_CHAINS[chain][0]
    return pwchain(pwchain_input()[:, :cin], pwchain_layers(chain))


def pwchain_check(chain, P, y):
    ref = pwchain_ref(chain)[:P]
    return Check(f"pwchain {chain} P={P}").add("y", y, ref, PW_CHAINS[chain][2] * max(1.0, ref.abs().max().item()))


# ------------------------------------------------------------------------------------------------ time attention, LayerNorm (+ residual)
A16_EPS = 1e-5
A16_DATA = ("unit", "flat")                                                # hash_normal; 0.5 + 0.01 hash_normal (per-pixel std 0.01: eps matters)
TA_CASES = [(1, 3), (5, 77), (9, 5)]                                       # T, n: T = 9 crosses the load loop's unroll of 8
TA_MAX_T = {384: 42, 256: 64}                                              # the largest T whose T * C * 4 bytes fit the 64 KiB of LDS (include/ppms.h)
LN16_PIXELS = 231                                                          # leaves a 4-pixel-block tail of 3


def _ln(x, w, b, eps, unbiased=False):
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=unbiased, keepdim=True)
    return (x - mean) * (var + eps).rsqrt() * w.double() + b.double()


def time_attn(x, w, b, eps=A16_EPS, unbiased=False, dh=None, heads=8):
    """x (T, n, C) -> (T, n, C) float64: per pixel, tokens = its T frames; y = LayerNorm(x); per head out_t = sum_t2 softmax_t2(y_t . y_t2 /
    sqrt(dh)) y_t2 with q = k = v = y (ppmtereo_update.py:603-606, :409-417).  dh: the head width of the scale (default C / heads)."""
    T, n, C = x.shape
    d = C // heads
    y = _ln(x.double().transpose(0, 1), w, b, eps, unbiased).reshape(n, T, heads, d).permute(0, 2, 1, 3)
    att = torch.softmax((y @ y.transpose(-2, -1)) * (dh or d) ** -0.5, dim=-1)
    return (att @ y).transpose(1, 2).reshape(n, T, C).transpose(0, 1)


def time_attn_f32(x, w, b, heads=8):
    T, n, C = x.shape
    d = C // heads
    y = F.layer_norm(x.float().transpose(0, 1), (C,), w.float(), b.float(), A16_EPS).reshape(n, T, heads, d).permute(0, 2, 1, 3)
    att = torch.softmax((y @ y.transpose(-2, -1)) * d ** -0.5, dim=-1)
    return (att @ y).transpose(1, 2).reshape(n, T, C).transpose(0, 1)


TA_WRONG = {"eps_1e-6": lambda x, w, b: time_attn(x, w, b, eps=1e-6), "unbiased": lambda x, w, b: time_attn(x, w, b, unbiased=True),
            "other_head_width": lambda x, w, b: time_attn(x, w, b, dh=48 if x.shape[2] == 256 else 32)}


def _a16_data(shape, seed, data):
    x = hash_normal(shape, seed)
    return (0.5 + 0.01 * x).float() if data == "flat" else x


@functools.lru_cache(maxsize=None)
def time_attn_inputs(C, case, data):
    T, n = case
    seed = 8400 + C + 10 * (TA_CASES.index(case) if case in TA_CASES else len(TA_CASES))      # (else: the largest accepted T, one pixel)
    return sp_round(_a16_data((T, n, C), seed, data)), 1.0 + 0.1 * hash_normal((C,), seed + 1), 0.1 * hash_normal((C,), seed + 2)


def time_attn_check(C, case, data, y):
    x, w, b = time_attn_inputs(C, case, data)
    ref = time_attn(x, w, b)
    return Check(f"time_attn C={C} T,n={case} {data}").add("y", y, ref, tol_reduce(ref, time_attn_f32(x, w, b), True))


def layernorm16(x, w, b, res=None, eps=A16_EPS, unbiased=False):
    """x (P, C), res (P, C) or None -> res + LayerNorm(x) float64, eps 1e-5 (attention.py:186-190)"""
    y = _ln(x.double(), w, b, eps, unbiased)
    return y if res is None else y + res.double()


def layernorm16_f32(x, w, b, res=None):
    y = F.layer_norm(x.float(), (x.shape[1],), w.float(), b.float(), A16_EPS)
    return y if res is None else y + res.float()


LN16_WRONG = {"eps_1e-6": lambda x, w, b, r: layernorm16(x, w, b, r, eps=1e-6), "unbiased": lambda x, w, b, r: layernorm16(x, w, b, r, unbiased=True),
              "residual_lo_plane_ignored": lambda x, w, b, r: None if r is None else layernorm16(x, w, b, r.to(torch.bfloat16).float())}


@functools.lru_cache(maxsize=None)
def layernorm16_inputs(C, data):
    """x, w, b and the residual as split bf16 holds it"""
    seed = 8500 + C
    return (_a16_data((LN16_PIXELS, C), seed, data), 1.0 + 0.1 * hash_normal((C,), seed + 1), 0.1 * hash_normal((C,), seed + 2),
            sp_round(hash_normal((LN16_PIXELS, C), seed + 3)))


def layernorm16_check(C, data, with_res, y):
    x, w, b, res = layernorm16_inputs(C, data)
    r = res if with_res else None
    ref = layernorm16(x, w, b, r)
    return Check(f"layernorm C={C} {data} res={int(with_res)}").add("y", y, ref, tol_reduce(ref, layernorm16_f32(x, w, b, r), True))


# ------------------------------------------------------------------------------------------------ linear attention
LA_EPS = 1e-6
LA_SPLITS, LA_PASS = 4, 160                                                # pixel splits of the kv kernel; pixels it stages per pass
LA_CASES = [(1, 3), (2, 77), (1, 644)]                                     # T, n: split 3 empty; a 32-pixel apply tail of 13; share 161 = one pass + 1
LA_DATA = ("unit", "tiny")                                                 # tiny: K x 1e-6, Q . sum K a few 1e-3 and less: the 1e-6 of the divisor shows


def linear_attention(Q, K, V, eps=LA_EPS, times_n=True, keep=None):
    """Q, K, V (T, n, heads, dh), Q and K already elu() + 1, V already / n -> (Q KV) / (Q . sum K + 1e-6) n float64 (attention.py:73-100).
    keep: (n,) mask of the source pixels the sums run over (the wrong variants)."""
    Q, K, V = Q.double(), K.double(), V.double()
    n = Q.shape[1]
    if keep is not None:
        K, V = K * keep.reshape(1, n, 1, 1), V * keep.reshape(1, n, 1, 1)
    KV = torch.einsum("nshd,nshv->nhdv", K, V)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(1)) + eps)
    out = torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z)
    return out * n if times_n else out


def linear_attention_f32(Q, K, V):
    """oracle.ppm_oracle.loftr_layer's expression in fp32"""
    Q, K, V = Q.float(), K.float(), V.float()
    KV = torch.einsum("nshd,nshv->nhdv", K, V)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(1)) + 1e-6)
    return torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * Q.shape[1]


def _la_keep(n, what):
    per = (n + LA_SPLITS - 1) // LA_SPLITS
    s = torch.arange(n)
    keep = (s < (LA_SPLITS - 1) * per) if what == "last_split" else ((s % per) < LA_PASS)
    return None if bool(keep.all()) else keep.double()                      # None: the variant does not apply to this n


def _la_with_keep(what):
    def fn(Q, K, V):
        keep = _la_keep(Q.shape[1], what)
        return None if keep is None else linear_attention(Q, K, V, keep=keep)
    return fn


LA_WRONG = {"no_divisor_eps": lambda Q, K, V: linear_attention(Q, K, V, eps=0.0), "last_split_dropped": _la_with_keep("last_split"),
            "first_pass_only": _la_with_keep("first_pass"), "times_n_omitted": lambda Q, K, V: linear_attention(Q, K, V, times_n=False)}


@functools.lru_cache(maxsize=None)
def linattn_inputs(dh, case, data):
    T, n = case
    seed = 8600 + dh + 10 * LA_CASES.index(case)
    shape = (T, n, 8, dh)
    Q, K = F.elu(hash_normal(shape, seed)) + 1, F.elu(hash_normal(shape, seed + 1)) + 1
    if data == "tiny":
        K = (K * 1e-6).float()
    return Q, K, hash_normal(shape, seed + 2) / n


def linattn_check(dh, case, data, y, label=None):
    Q, K, V = linattn_inputs(dh, case, data)
    ref = linear_attention(Q, K, V)
    return Check(label or f"linear_attention dh={dh} T,n={case} {data}").add("y", y, ref, tol_reduce(ref, linear_attention_f32(Q, K, V), True))


# ================================================================================================ memory read-out
# The pick-and-play chain (mem_pick.hip: qk_pool / qk_cos, the QAM pick, the operand kernels; mem_attn.hip): tests/test_gpu_memory_ops.py.
# Similarity, score and s_hat are reductions (kind c); SEL and the usage counter are exact; the operands are one fp32 operation rounded to
# bf16 (exact: the build does not contract a * s + p, -ffp-contract=off); the read-out keeps the per-element bound tests/test_gpu_ops.py
# derives for it, restated here against the float64 read-out.
MEM_SCALE = 128 ** -0.5 * math.log(256, 12000)                            # engine.softmax_scale(128), ppmstereo.py:494


# ------------------------------------------------------------------------------------------------ frame similarity
SIM_CASES = [(1, 4, 4), (2, 5, 7), (3, 10, 18), (5, 8, 32), (9, 13, 22), (2, 23, 40)]      # T, H, W: one cell; one cell row of unequal windows; ...
SIM_EXTRA = 3                                                              # the inputs hold Tg = T + 3 frames: the other ranks' of a sharded window
SIM_DATA = ("unit", "edge")                                                # edge: frame 0 constant zero (norm 0: the eps branch), frame 1 x 1e-6


def _windows(n, o, adaptive=True):
    """torch's adaptive windows: [floor(i n / o), ceil((i + 1) n / o)); or fixed windows of 4 that drop the remainder"""
    return [((i * n) // o, -((-(i + 1) * n) // o)) for i in range(o)] if adaptive else [(4 * i, 4 * i + 4) for i in range(o)]


def qk_pool(x, pool="max", adaptive=True, mean_first=False):
    """x (T, H, W, 128) -> (T, (H // 4) (W // 4)) float64: the maximum of every channel over the adaptive window, then the mean over the
    channels (ppmstereo.py:397-423).  The keyword arguments are the wrong variants."""
    T, H, W, C = x.shape
    OH, OW = H // 4, W // 4
    x = x.double()
    out = torch.empty(T, OH, OW, dtype=F64)
    for oy, (ys, ye) in enumerate(_windows(H, OH, adaptive)):
        for ox, (xs, xe) in enumerate(_windows(W, OW, adaptive)):
            win = x[:, ys:ye, xs:xe].reshape(T, -1, C)
            if mean_first:
                out[:, oy, ox] = win.mean(2).max(1).values                 # the channel mean of every pixel, then the window's maximum
            elif pool == "avg":
                out[:, oy, ox] = win.mean(1).mean(1)
            else:
                out[:, oy, ox] = win.max(1).values.mean(1)
    return out.reshape(T, OH * OW)


def qk_cos(qbar, kbar, eps_each=True, transposed=False):
    """sim[i][j] = cos(kbar_i, qbar_j), each norm clamped at 1e-8 (F.cosine_similarity)"""
    a, b = (qbar.double(), kbar.double()) if transposed else (kbar.double(), qbar.double())
    na, nb = a.norm(dim=1)[:, None], b.norm(dim=1)[None]
    den = na.clamp_min(1e-8) * nb.clamp_min(1e-8) if eps_each else (na * nb).clamp_min(1e-8)
    return (a @ b.t()) / den


def qk_similarity(q, k, pool_kw=None, cos_kw=None):
    """q, k (T, H, W, 128) -> qbar, kbar (T, cells), sim (T, T) float64"""
    qbar, kbar = qk_pool(q, **(pool_kw or {})), qk_pool(k, **(pool_kw or {}))
    return qbar, kbar, qk_cos(qbar, kbar, **(cos_kw or {}))


def qk_similarity_f32(q, k):
    """oracle.ppm_oracle.qk_similarity's op sequence in fp32"""
    T, H, W, C = q.shape
    pool = lambda x: F.adaptive_max_pool2d(x.float().permute(0, 3, 1, 2), (H // 4, W // 4)).mean(1).reshape(T, -1)
    qbar, kbar = pool(q), pool(k)
    return qbar, kbar, F.cosine_similarity(qbar.unsqueeze(0), kbar.unsqueeze(1), dim=-1)


SIM_WRONG = {
    "transposed": dict(cos_kw=dict(transposed=True)), "average_pool": dict(pool_kw=dict(pool="avg")),
    "fixed_4x4_windows": dict(pool_kw=dict(adaptive=False)), "mean_before_max": dict(pool_kw=dict(mean_first=True)),
    "eps_on_the_product": dict(cos_kw=dict(eps_each=False)),
}


@functools.lru_cache(maxsize=None)
def sim_inputs(case, data):
    """q, k (T + 3, H, W, 128) fp32; k shares 0.3 of q, so the similarities are not all near 0"""
    T, H, W = case
    seed = 9000 + 10 * SIM_CASES.index(case)
    q = hash_normal((T + SIM_EXTRA, H, W, 128), seed)
    k = (hash_normal((T + SIM_EXTRA, H, W, 128), seed + 1) + 0.3 * q).float()
    if data == "edge":
        q[0], k[0] = 0.0, 0.0
        q[1], k[1] = q[1] * 1e-6, k[1] * 1e-6
    return q, k


@functools.lru_cache(maxsize=None)
def sim_refs(case, data, frames):
    """(reference, fp32 torch) of the first `frames` frames: each (qbar, kbar, sim)"""
    q, k = sim_inputs(case, data)
    return qk_similarity(q[:frames], k[:frames]), qk_similarity_f32(q[:frames], k[:frames])


def sim_check(case, data, frames, sim, pooled=None, label=None):
    """sim (frames, frames); pooled (2, frames, cells) or None"""
    ref, f32 = sim_refs(case, data, frames)
    ck = Check(label or f"qk_similarity {case} {data} frames={frames}")
    if pooled is not None:
        ck.add("qbar", pooled[0], ref[0], tol_reduce(ref[0], f32[0], False)).add("kbar", pooled[1], ref[1], tol_reduce(ref[1], f32[1], False))
    return ck.add("sim", sim, ref[2], tol_reduce(ref[2], f32[2], False))


# ------------------------------------------------------------------------------------------------ QAM pick
TOP_K = 5
PICK_ITERS = 6                                                             # consecutive picks with the evolving usage counter
PICK_CASES = {1: 1, 2: 3, 4: 64, 5: 80, 6: 1, 8: 3, 9: 65, 16: 64, 17: 80, 40: 130, 64: 65}      # T -> nblk.  T > 8: the second group of eight
#   frames of the confidence sums; nblk > 64: a lane takes a second block; 9 / 65 and 40 / 130 have both at once; 40: the window of BASELINE
#   config 4; 64: the documented maximum (48 KiB of dynamic LDS, bit 63 of the masks)
PICK_SEEDS = {1: 9100, 2: 9110, 4: 9120, 5: 9130, 6: 9140, 8: 9150, 9: 9160, 16: 9170, 17: 9180, 40: 9197, 64: 9205}     # chosen so that
#   pick_near_tie holds on every row (tests/test_kernel_refs.py asserts it): a seed that fails is replaced, no row is left out
PICK_TIES = {  # T, tied frames, frames every clip picks first, frames picked, iterations -- an exact tie that straddles rank 5 / 6
    "pair": (8, (2, 6), (0, 3, 5, 7), (0, 2, 3, 5, 7)),
    "triple_two_in": (9, (1, 4, 8), (0, 2, 5), (0, 1, 2, 4, 5)),
    "triple_one_in": (17, (3, 9, 16), (0, 5, 11, 12), (0, 3, 5, 11, 12)),
}
TIE_NBLK, TIE_HW = 3, 700


def pick_hw(nblk):
    """pixels of a map with nblk blocks of 256, the last one partly filled"""
    return 256 * nblk - 68


def qam_pick(sim, strive, part, HW, dtype=F64, plus_T=True, pen_axis=1, conf_op="add", shat_over="picked", count="picked", order="ascending",
             divisor=None, ties="lowest"):
    """sim, strive (T, T), part (T, nblk) block sums of the uncertainty map -> score (T, T), sel (T, 5) int64 ascending, shat (T, 5), the new
    counter (T, T).  conf_j = sum_b part[j][b] / HW; score_ij = exp(-S_ij / (sum_j S_ij + T)) sim_ij + conf_j; the pick of row i: its
    min(5, T) highest scores, the lowest frame index first among equal ones; S_i,picked += 1; shat = score_i,picked / mean(score_i,picked)
    (ppmstereo.py:501-513, 532-533).  Slots >= min(5, T) hold 0.  dtype = float32: the plain-torch form.  The other keyword arguments are
    the wrong variants."""
    T = sim.shape[0]
    sim, strive, part = sim.to(dtype), strive.to(dtype), part.to(dtype)
    conf = part.sum(1) / (HW if divisor is None else divisor)
    pen = torch.exp(-strive / (strive.sum(pen_axis, keepdim=True) + (T if plus_T else 0)))
    score = pen * sim * conf[None] if conf_op == "mul" else pen * sim + conf[None]
    k = min(TOP_K, T)
    if ties == "lowest":
        idx = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :k]
    else:
        idx = T - 1 - torch.sort(score.flip(1), dim=1, descending=True, stable=True).indices[:, :k]
    if order == "ascending":
        idx = idx.sort(1).values
    s = torch.gather(score, 1, idx)
    shat = s / (score.mean(1, keepdim=True) if shat_over == "all" else s.mean(1, keepdim=True))
    new = strive + 1 if count == "all" else strive.clone().scatter_add_(1, idx, torch.ones_like(s))
    sel = torch.zeros(T, 5, dtype=torch.int64)
    sh = torch.zeros(T, 5, dtype=dtype)
    sel[:, :k], sh[:, :k] = idx, shat
    return score, sel, sh, new


PICK_WRONG = {
    "penalty_without_T": dict(plus_T=False), "penalty_over_the_other_axis": dict(pen_axis=0), "confidence_multiplied": dict(conf_op="mul"),
    "shat_over_all_frames": dict(shat_over="all"), "counter_for_every_frame": dict(count="all"), "sel_in_score_order": dict(order="score"),
    "confidence_over_nblk_256": dict(divisor="nblk256"), "ties_to_the_highest_index": dict(ties="highest"),
}


def _block_sums(T, nblk, HW, seed):
    """fp32 (T, nblk): 256 x a sigmoid per block (the sum of 256 uncertainties), the last block scaled to its pixel count"""
    part = 256.0 * torch.sigmoid(hash_normal((T, nblk), seed))
    part[:, -1] *= (HW - 256 * (nblk - 1)) / 256.0
    return part.float()


@functools.lru_cache(maxsize=None)
def pick_inputs(T):
    """sim (T, T) = tanh(hash_normal) (T = 1: NaN, as the product's is there), [part (T, nblk)] per iteration, HW"""
    nblk, seed = PICK_CASES[T], PICK_SEEDS[T]
    HW = pick_hw(nblk)
    sim = torch.tanh(hash_normal((T, T), seed))
    if T == 1:
        sim.fill_(float("nan"))
    return sim, tuple(_block_sums(T, nblk, HW, seed + 1 + it) for it in range(PICK_ITERS)), HW


def pick_sequence(T, **wrong):
    """the PICK_ITERS consecutive picks from a counter of ones: per iteration (counter before, reference, fp32 torch) -- both fed the
    reference's counter (small integers: exact in either type) -- or, with a wrong variant, (counter before, its result) evolving its own"""
    sim, parts, HW = pick_inputs(T)
    if wrong.get("divisor") == "nblk256":
        wrong = dict(wrong, divisor=PICK_CASES[T] * 256)
    strive, out = torch.ones(T, T, dtype=F64), []
    for part in parts:
        if wrong:
            res = qam_pick(sim, strive, part, HW, **wrong)
            out.append((strive, res))
        else:
            res = qam_pick(sim, strive, part, HW)
            out.append((strive, res, qam_pick(sim, strive, part, HW, dtype=torch.float32)))
        strive = res[3]
    return out


@functools.lru_cache(maxsize=None)
def pick_refs(T):
    return tuple(pick_sequence(T))


def pick_near_tie(T):
    """(the smallest float64 gap between the 5th and the 6th score over every iteration and row, the largest |fp32 - float64| score of the
    case): the pick is safe from an ulp of expf where the first is at least 256 x the second"""
    gap, err = math.inf, 0.0
    for _, ref, f32 in pick_refs(T):
        if T > TOP_K:
            s = ref[0].sort(1, descending=True).values
            gap = min(gap, (s[:, TOP_K - 1] - s[:, TOP_K]).min().item())
        if T > 1:
            err = max(err, (f32[0].double() - ref[0]).abs().max().item())
    return gap, err


def pick_check(T, it, score, sel, shat, strive_new, label=None, ck=None):
    """one iteration's results against the reference; score and shat by tol_reduce of that iteration: 8 x the fp32-torch error of the same
    pick on the same input (T = 1: NaN scores; frame 0 is picked, the counter counts)"""
    _, ref, f32 = pick_refs(T)[it]
    ck = ck or Check(label or f"qam pick T={T}")
    ck.exact(f"sel[{it}]", sel.long(), ref[1]).exact(f"counter[{it}]", strive_new.double(), ref[3])
    if T == 1:
        bad = float(not (torch.isnan(score).all() and torch.isnan(shat[:, 0]).all() and (shat[:, 1:] == 0).all()))
        ck.items.append((f"nan[{it}]", bad, 0.0))
        return ck
    return ck.add(f"score[{it}]", score, ref[0], tol_reduce(ref[0], f32[0], False)).add(f"shat[{it}]", shat, ref[2], tol_reduce(ref[2], f32[2], False))


@functools.lru_cache(maxsize=None)
def tie_inputs(name):
    """sim, counter, part with bit-equal columns / rows at the tied frames; the frames of `first` carry confidence ~10, the tied ones ~5,
    the rest ~0.5, so that in every row the tie occupies the ranks from len(first) + 1 on"""
    T, tied, first, _ = PICK_TIES[name]
    seed = 9300 + 10 * list(PICK_TIES).index(name)
    sim = torch.tanh(hash_normal((T, T), seed))
    strive = 1.0 + torch.floor(3.0 * torch.sigmoid(hash_normal((T, T), seed + 1)))
    part = _block_sums(T, TIE_NBLK, TIE_HW, seed + 2)
    part[list(first)] += 10.0 * TIE_HW / TIE_NBLK
    part[list(tied)] += 5.0 * TIE_HW / TIE_NBLK
    for t in tied[1:]:
        sim[:, t], strive[:, t], part[t] = sim[:, tied[0]], strive[:, tied[0]], part[tied[0]]
    return sim, strive, part.float()


def tie_check(name, score, sel, shat, strive_new, label=None):
    sim, strive, part = tie_inputs(name)
    T, tied, first, picked = PICK_TIES[name]
    ref = qam_pick(sim, strive, part, TIE_HW)
    f32 = qam_pick(sim, strive, part, TIE_HW, dtype=torch.float32)
    ck = Check(label or f"qam pick tie {name}")
    ck.exact("sel", sel.long(), torch.tensor(picked).expand(T, 5)).exact("sel=ref", sel.long(), ref[1]).exact("counter", strive_new.double(), ref[3])
    return ck.add("score", score, ref[0], tol_reduce(ref[0], f32[0], False)).add("shat", shat, ref[2], tol_reduce(ref[2], f32[2], False))


# ------------------------------------------------------------------------------------------------ attention operands
PREP_N = [1, 5, 64, 100]
PREP_LD = (128, 256)
PREP_KSEL = (1, 3, 5)
PREP_T, PREP_TG = 2, 7                                                     # clips of this rank, frames of the window (the sharded form)


def prep_q(q, pe):
    """q (T, n, 128), pe (T, 128) fp32 -> bf16(q + pe): one fp32 addition (ppmstereo.py:518-522)"""
    return (q.float() + pe.float()[:, None]).to(torch.bfloat16)


def prep_k(key, pe, sel, shat, ksel):
    """key (Tg, n, 128), pe (Tg, 128), sel (T, 5), shat (T, 5) -> (T, ksel, n, 128) bf16(key[sel] * shat + pe[sel]): an fp32 product rounded,
    then an fp32 sum rounded (ppmstereo.py:541, 547)"""
    J = sel[:, :ksel].long()
    return (key.float()[J] * shat.float()[:, :ksel, None, None] + pe.float()[J][:, :, None]).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def prep_inputs(n):
    """q, key (Tg, n, 128), pe (Tg, 128) -- finite, unlike temporal_pe at T = 1 --, sel (T, 5) rows ascending over the Tg frames, shat (T, 5)"""
    seed = 9400 + n
    q, key = hash_normal((PREP_TG, n, 128), seed), hash_normal((PREP_TG, n, 128), seed + 1)
    pe = torch.sin(hash_normal((PREP_TG, 128), seed + 2) * 3.0)
    sel = torch.tensor([[1, 2, 4, 5, 6], [0, 3, 4, 5, 6]], dtype=torch.int32)
    shat = (1.0 + 0.3 * torch.tanh(hash_normal((PREP_T, 5), seed + 3))).float()
    return q, key, pe.float(), sel, shat


# ------------------------------------------------------------------------------------------------ memory attention
ATTN_BETA = 0.5
ATTN32_T, ATTN32_N, ATTN32_KSEL = 2, [4, 20, 36, 60, 72, 100], (1, 3, 5)   # 60: n % 8 != 0 (element-wise V loads); 72: vector rows, a partial tile
ATTN64_T, ATTN64_N, ATTN64_KSEL = 3, [64, 128, 192, 320], (1, 2, 3, 4, 5)  # 1, 2, 3 and 5 key tiles per frame; waves without a query
ATTN64_FRAMES = (0, 1, 2, 3, 4, 5)                                         # frames_per_workgroup, values above ksel included
ATTN_SHARDED = {32: (2, 6, 100, 3, ((1, 3, 5), (0, 2, 5))), 64: (2, 6, 128, 3, ((1, 3, 5), (0, 2, 5)))}      # kernel -> T clips, Tg frames of vt, n, ksel, sel
FIXUP_T, FIXUP_N, FIXUP_KSEL, FIXUP_SLOT, FIXUP_FRAMES = 2, 320, 5, 2, (1, 2, 3)


def attn_eps_p(p_format):
    """half an ulp of the format the probabilities are rounded to: 2^-8 (bf16), 2^-11 (fp16)"""
    return 2.0 ** -11 if p_format == 1 else 2.0 ** -8


def mem_attn(q, k, v, sel, ksel, scale, v_from="sel", softmax="joint", pad_keys=False):
    """q (T, n, 128), k (T, ksel, n, 128), v (Tg, 128, n) -- the values the 16-bit operands hold --, sel (T, 5) -> x (T, n, 128) float64 =
    softmax(Q K^T scale) V over the ksel n keys of the picked frames, and P |V| (T, n, 128), the weight of the probability rounding in
    the bound.  The keyword arguments are the wrong variants."""
    T, n, _ = q.shape
    xs, pvs = [], []
    for i in range(T):
        J = [int(sel[i, s]) if v_from == "sel" else s for s in range(ksel)]
        Q, K = q[i].double(), k[i].double()                               # (n, 128), (ksel, n, 128)
        V = torch.stack([v[j].double().t() for j in J])                   # (ksel, n, 128)
        if pad_keys:                                                      # the keys up to the next multiple of 64: zero keys, zero values
            pad = -n % 64
            K, V = F.pad(K, (0, 0, 0, pad)), F.pad(V, (0, 0, 0, pad))
        S = torch.einsum("qc,skc->qsk", Q, K) * scale                     # (n, ksel, keys)
        if softmax == "joint":
            P = torch.softmax(S.reshape(n, -1), dim=-1).reshape(S.shape)
        else:                                                             # per frame, then averaged: the 2^(m_s - m) l_s weights left out
            P = torch.softmax(S, dim=-1) / ksel
        xs.append(torch.einsum("qsk,skc->qc", P, V))
        pvs.append(torch.einsum("qsk,skc->qc", P, V.abs()))
    return torch.stack(xs), torch.stack(pvs)


def mem_attn_f32(q, k, v, sel, ksel, scale):
    """oracle.ppm_oracle.flash_attn_math's op sequence: fp32 softmax and product on the 16-bit operands, bf16 result"""
    out = []
    for i in range(q.shape[0]):
        K = k[i].float().reshape(-1, 128)
        V = torch.cat([v[int(sel[i, s])].float().t() for s in range(ksel)], 0)
        out.append((torch.softmax((q[i].float() @ K.t()) * scale, dim=-1) @ V).to(torch.bfloat16))
    return torch.stack(out)


def mfg_of(mf, hid, beta=ATTN_BETA):
    """mf (T n, 128), hid (T, n, 128) bf16 -> mf + beta hid, float64"""
    return mf.double() + beta * hid.float().double().reshape(mf.shape)


ATTN_WRONG = {
    "v_from_slot": dict(kw=dict(v_from="slot")), "per_frame_softmax_averaged": dict(kw=dict(softmax="per_frame")),
    "tail_keys_unmasked": dict(kw=dict(pad_keys=True), needs_tail=True), "scale_without_log2e": dict(scale=math.log(2.0)),
    "scale_with_log2e_twice": dict(scale=1.0 / math.log(2.0)), "beta_dropped": dict(beta=1.0), "hid_rounded_before_the_division": dict(round_first=True),
}


def mem_attn_wrong(name, case):
    """(hid bf16, mfg float64) of a wrong variant on the inputs attn_named_inputs(*case), or None where it does not apply"""
    w = ATTN_WRONG[name]
    (q, k, v, sel, ksel, mf), scale = attn_named_inputs(*case)
    if w.get("needs_tail") and q.shape[1] % 64 == 0:
        return None
    if w.get("round_first"):                                              # O = P~ V and l = sum P~ with P~ = exp(S - max); bf16(O) / l
        x, _ = mem_attn(q, k, v, sel, ksel, scale)
        S = torch.einsum("tqc,tskc->tqsk", q.double(), k.double()).reshape(q.shape[0], q.shape[1], -1) * scale
        l = torch.exp(S - S.max(-1, keepdim=True).values).sum(-1, keepdim=True)
        hid = ((x * l).float().to(torch.bfloat16).double() / l).float().to(torch.bfloat16)
    else:
        hid = mem_attn(q, k, v, sel, ksel, scale * w.get("scale", 1.0), **w.get("kw", {}))[0].float().to(torch.bfloat16)
    return hid, mfg_of(mf, hid, w.get("beta", ATTN_BETA))


def _v16(x):
    """x rounded to bf16, as fp32; the few values too small for fp16 to hold exactly (|v| < 2^-14, off its 2^-24 grid) become 0, so that the
    bf16 and the fp16 image of V^T (ppms_mem_attn's two p_formats) hold the same numbers and one reference serves both"""
    v = x.to(torch.bfloat16).float()
    return torch.where(v.half().float() == v, v, torch.zeros_like(v))


def _attn_sel(T, Tg, ksel, seed):
    """(T, 5) int32: per clip ksel distinct frames of the Tg, ascending; no row is the identity 0 .. ksel - 1"""
    g = torch.Generator().manual_seed(seed)
    sel = torch.zeros(T, 5, dtype=torch.int32)
    for i in range(T):
        while True:
            row = torch.randperm(Tg, generator=g)[:ksel].sort().values
            if row.tolist() != list(range(ksel)):
                break
        sel[i, :ksel] = row.int()
    return sel


@functools.lru_cache(maxsize=None)
def attn_inputs(T, Tg, n, ksel, rows=None):
    """q (T, n, 128), k (T, ksel, n, 128), v (Tg, 128, n): hash_normal rounded to bf16 (what the operand buffers hold); sel (T, 5); ksel;
    mf (T n, 128) as split bf16 holds it"""
    seed = 9500 + 7 * n + ksel + 100 * Tg
    r = lambda shape, s: hash_normal(shape, s).to(torch.bfloat16).float()
    sel = _attn_sel(T, Tg, ksel, seed + 3)
    if rows is not None:
        sel[:, :ksel] = torch.tensor(rows, dtype=torch.int32)
    return (r((T, n, 128), seed), r((T, ksel, n, 128), seed + 1), _v16(hash_normal((Tg, 128, n), seed + 2)), sel, ksel,
            sp_round(hash_normal((T * n, 128), seed + 4)))


@functools.lru_cache(maxsize=None)
def fixup_inputs():
    """test_mem_attn_sharp_softmax's construction, confined to one tile: the keys are 0.1 hash_normal; every query i of the partly filled second
    256-query block of clip 0 has ONE key, in slot 2, that carries 40 x the unit vector of the query's channels 64-127, and the queries of
    the first block are zero in those channels (they meet the boosted keys with a score of exactly 0 from them).  Clip 1 has no such key.
    scale = 1: the boosted score is ~650 log2 units above the others."""
    T, n, ksel = FIXUP_T, FIXUP_N, FIXUP_KSEL
    q = hash_normal((T, n, 128), 9600)
    k = hash_normal((T, ksel, n, 128), 9601) * 0.1
    q[:, :256, 64:] = 0.0
    for i in range(256, n):
        u = q[0, i].clone()
        u[:64] = 0.0
        k[0, FIXUP_SLOT, (i * 7 + 300) % n] += 40.0 * u / u.norm()
    r = lambda t: t.to(torch.bfloat16).float()
    q, k = r(q), r(k)
    assert (q[:, :256, 64:] == 0).all()
    v = _v16(hash_normal((ksel + 1, 128, n), 9602))
    return q, k, v, _attn_sel(T, ksel + 1, ksel, 9603), ksel, sp_round(hash_normal((T * n, 128), 9604))


def attn_named_inputs(kind, *args):
    """("table", kernel, n, ksel): a case of the 32- / 64-query tables -- vt holds max(T, ksel + 1) frames, so that no sel row is the identity;
    ("sharded", kernel): T clips of this rank, sel rows over the Tg frames of vt; ("fixup",): fixup_inputs.  -> (inputs, softmax scale)"""
    if kind == "table":
        kernel, n, ksel = args
        T = ATTN32_T if kernel == 32 else ATTN64_T
        return attn_inputs(T, max(T, ksel + 1), n, ksel), MEM_SCALE
    if kind == "sharded":
        return attn_inputs(*ATTN_SHARDED[args[0]]), MEM_SCALE
    return fixup_inputs(), 1.0


@functools.lru_cache(maxsize=None)
def attn_ref(kind, *args):
    """(x, P |V|) of the named inputs: computed once, shared by the formats and launch forms of the case"""
    inp, scale = attn_named_inputs(kind, *args)
    return mem_attn(*inp[:5], scale)


def attn_check(name, p_format, raw, mfg, label=None):
    """name: the arguments of attn_named_inputs; raw (T, n, 128) bf16 hid, mfg (T n, 128) fp32 (hi + lo).  Per element |raw - x| <=
    eps_P (P |V|) (the probabilities rounded to the P~ format before the product, all errors aligned) + 2^-8 |x| (the bf16 result: half an
    ulp) + 1e-6; per clip the mean error at most half the mean bound (rounding errors do not line up: the final rounding alone averages ~0.35 of
    its term); mfg = mf + beta raw as split bf16."""
    x, pv = attn_ref(*name)
    mf = attn_named_inputs(*name)[0][5]
    bound = attn_eps_p(p_format) * pv + 2.0 ** -8 * x.abs() + 1e-6
    ck = Check(label or f"mem_attn {name} p_format={p_format}")
    got = raw.detach().cpu().float().double()
    finite = got.shape == x.shape and bool(torch.isfinite(got).all())
    ck.items.append(("hid/bound", ((got - x).abs() / bound).max().item() if finite else math.inf, 1.0))
    ck.items.append(("mean", ((got - x).abs().mean((1, 2)) / bound.mean((1, 2))).max().item() if finite else math.inf, 0.5))      # per clip
    want = mfg_of(mf, raw.detach().cpu())
    return ck.add("mfg", mfg, want, tol_sp(want))


# ================================================================================================ correlation build, flow output
# The pyramid build (corr.hip: the line-resident kernel and the general one), the convex upsamplings and the tap gather-sum (loop_ops.hip),
# the bilinear resize and the four tiled transposes (glue_ops.hip): tests/test_gpu_flow_ops.py.  Pyramid levels, upsamplings and resize are
# kind (c); the transposes and the accum side of the gather-sum are exact; the gather-sum's out has an elementwise bound of its own.
# ------------------------------------------------------------------------------------------------ correlation pyramid
CORR_CASES = {  # B, C, H, W, features one float into their allocation
    "w32_c32": (1, 32, 9, 20, False),          # the 32-wide line kernel, nch = 2: 9 lines = one full group of 8 plus one; widths 10 / 5 / 2 / 1
    "w64_c48": (3, 48, 3, 44, False),          # the 64-wide one, nch = 3; widths 22 / 11 / 5 / 2: levels 3 and 4 drop a window
    "w128_c16": (1, 16, 10, 132, False),       # the 128-wide one, two x1 and two x2 blocks, the last 4 wide; an epilogue after every stage
    "w128_c64": (2, 64, 4, 260, False),        # three blocks, nch = 4, exactly 8 lines
    "general_w70": (1, 20, 9, 70, False),      # the general kernel: W % 4 != 0, C % 16 != 0, three tiles on four waves, the regrouped branch
    "general_c7": (2, 7, 4, 18, False),        # odd C: the channel guard splits a pair of one MFMA
    "general_misaligned": (3, 48, 3, 44, True),      # the general kernel on a line-kernel shape
}
CORR_GAPS = (4, 8, 4, 8, 4)                                                # sentinel floats after each level of the pyramid buffer


def corr_pyramid(f1, f2, dtype=F64, swap=False, div_c=False, ceil=False, offset1=False, lines_xor1=False, late_window=False):
    """f1, f2 (B, C, H, W) -> 5 levels (B H W, W >> l): vol[b, y, x1, x2] = sum_c f1[b, c, y, x1] f2[b, c, y, x2] / sqrt(C), then four times
    0.5 (even + odd) along x2 with floored widths (corr.py:56-72, 96-104).  dtype = float32: the plain-torch form.  The other keyword
    arguments are the wrong variants."""
    B, C, H, W = f1.shape
    vol = torch.einsum("bcyi,bcyj->byij", f1.to(dtype), f2.to(dtype)) / (C if div_c else math.sqrt(C))
    if swap:
        vol = vol.transpose(2, 3)
    if lines_xor1:                                                          # lines r and r ^ 1 exchanged inside every full group of 8 lines
        r = torch.arange(B * H)
        r = torch.where(r < (B * H) // 8 * 8, r ^ 1, r)
        vol = vol.reshape(B * H, W, W)[r]
    lvl = vol.reshape(B * H * W, W)
    pyr = [lvl]
    for l in range(1, 5):
        if late_window:                                                     # pooled from level 0, every window one element late
            w, k = W >> l, 1 << l
            lvl = F.pad(pyr[0], (0, k))[:, 1:1 + w * k].reshape(-1, w, k).mean(2)
        else:
            src = F.pad(lvl, (0, 2))
            w = (lvl.shape[1] + 1) // 2 if ceil else lvl.shape[1] // 2      # ceil: the incomplete last window kept (its missing half is 0)
            o = 1 if offset1 else 0
            lvl = 0.5 * (src[:, o:o + 2 * w:2] + src[:, o + 1:o + 1 + 2 * w:2])
        pyr.append(lvl)
    return pyr


def corr_pyramid_f32(f1, f2):
    return corr_pyramid(f1, f2, dtype=torch.float32)


CORR_WRONG = {"x1_x2_swapped": dict(swap=True), "divided_by_C": dict(div_c=True), "ceil_widths": dict(ceil=True), "pairs_from_offset_1": dict(offset1=True),
              "lines_r_and_r^1_exchanged": dict(lines_xor1=True), "pooled_from_level_0_one_late": dict(late_window=True)}


@functools.lru_cache(maxsize=None)
def corr_inputs(case):
    """f1, f2 (B, C, H, W) fp32: 0.5 + s_c hash_normal with the per-channel scales s_c spread geometrically over 0.25 .. 4"""
    B, C, H, W, _ = CORR_CASES[case]
    seed = 9700 + 10 * list(CORR_CASES).index(case)
    s = (0.25 * 16.0 ** (torch.arange(C, dtype=F64) * 3 % C / max(1, C - 1))).float().reshape(1, C, 1, 1)
    return (0.5 + s * hash_normal((B, C, H, W), seed)).float(), (0.5 + s * hash_normal((B, C, H, W), seed + 1)).float()


@functools.lru_cache(maxsize=None)
def corr_refs(case):
    f1, f2 = corr_inputs(case)
    return tuple(corr_pyramid(f1, f2)), tuple(corr_pyramid_f32(f1, f2))


def corr_check(case, levels, label=None):
    """levels: 5 x (B H W, W >> l)"""
    ref, f32 = corr_refs(case)
    ck = Check(label or f"corr_build {case}")
    for l in range(5):
        ck.add(f"level{l}", levels[l], ref[l], tol_reduce(ref[l], f32[l], False))
    return ck


# ------------------------------------------------------------------------------------------------ convex upsampling
CONVEX_HALO = 2                                                            # halo frames on each side of the flow buffer, as the engine's
CONVEX2D_CASES = [(2, 5, 7, 144), (3, 6, 10, 160), (1, 1, 1, 152)]          # BT, H, W, mask_ld
CONVEX3D_CASES = [(1, 4, 6, 0, 432), (3, 5, 9, 0, 440), (2, 5, 9, 1, 432), (4, 3, 5, 2, 432)]      # T, H, W, t_halo, mask_ld
CONVEX_DATA = ("unit", "sharp", "bigflow")                                 # N(0, 1) logits; 100 + 30 N(0, 1): exp without the max overflows fp32; |flow| ~ 60


def convex_upsample_3d(flow, mask, t_halo, kt=3, dtype=F64, sub_max=True, in_range_only=False, swap_ky_kx=False, swap_i_j=False, pad="zeros",
                       factor=4.0, kt_fastest=False, halo_zero=False, one_beyond=False):
    """flow (T + 2 t_halo, H, W, 2), mask (T, H, W, 16 ntap), ntap = 9 kt -> (T, 2, 4 H, 4 W):
    out[t, c, 4 y + i, 4 x + j] = sum_k softmax_k(mask[t, y, x, 16 k + 4 i + j]) 4 flow[t + dt, y + dy, x + dx, c], k = (dt' 3 + dy') 3 + dx', zero
    outside the frame and beyond the t_halo frames around the T own ones (ppmstereo.py:185-228).  dtype = float32: the plain-torch form.  The
    other keyword arguments are the wrong variants."""
    T, H, W, ntap = mask.shape[0], mask.shape[1], mask.shape[2], 9 * kt
    m = mask.to(dtype).reshape(T, H, W, ntap, 4, 4)
    if sub_max:
        wgt = torch.softmax(m, dim=3)
    else:                                                                   # exp of the raw logits, in fp32 as a kernel would
        e = torch.exp(m.float())
        wgt = (e / e.sum(3, keepdim=True)).to(dtype)
    fl = factor * flow.to(dtype)
    th = t_halo
    if one_beyond:                                                          # the frame past the halo is read: NaN, as the buffer holds there
        fl, th = torch.cat([torch.full_like(fl[:1], math.nan), fl, torch.full_like(fl[:1], math.nan)]), t_halo + 1
    Tf = fl.shape[0]
    fp = fl.permute(0, 3, 1, 2)
    fp = (F.pad(fp, (1, 1, 1, 1), mode="replicate") if pad == "replicate" else F.pad(fp, (1, 1, 1, 1))).permute(0, 2, 3, 1)
    inside = F.pad(torch.ones(H, W, dtype=dtype), (1, 1, 1, 1))
    t = torch.arange(T)
    out = torch.zeros(T, H, W, 4, 4, 2, dtype=dtype)
    terms, oks = [], []
    for k in range(ntap):
        if kt_fastest:
            dt, dy, dx = k % kt - kt // 2, k // kt // 3 - 1, k // kt % 3 - 1
        else:
            dt, dy, dx = k // 9 - kt // 2, k // 3 % 3 - 1, k % 3 - 1
        if swap_ky_kx:
            dy, dx = dx, dy
        tt = t + dt
        ok_t = ((tt >= 0) & (tt < T)) if halo_zero else ((tt + th >= 0) & (tt + th < Tf))
        nb = fp[(tt + th).clamp(0, Tf - 1), 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]                        # (T, H, W, 2)
        nb = torch.where(ok_t.reshape(T, 1, 1, 1), nb, torch.zeros_like(nb))
        terms.append(nb)
        oks.append(ok_t.to(dtype).reshape(T, 1, 1) * inside[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
    if in_range_only:                                                       # renormalised over the taps that lie inside the volume
        ok = torch.stack(oks, 3)[..., None, None]
        wgt = wgt * ok / (wgt * ok).sum(3, keepdim=True)
    for k in range(ntap):
        out += wgt[:, :, :, k, :, :, None] * terms[k][:, :, :, None, None, :]
    if swap_i_j:
        out = out.transpose(3, 4)
    return out.permute(0, 5, 1, 3, 2, 4).reshape(T, 2, 4 * H, 4 * W)


def convex_upsample(flow, mask, **kw):
    """flow (BT, H, W, 2), mask (BT, H, W, 144) -> (BT, 2, 4 H, 4 W): the 9 taps of the frame itself"""
    return convex_upsample_3d(flow, mask, 0, kt=1, **kw)


def convex_upsample_f32(flow, mask):
    return convex_upsample(flow, mask, dtype=torch.float32)


def convex_upsample_3d_f32(flow, mask, t_halo):
    return convex_upsample_3d(flow, mask, t_halo, dtype=torch.float32)


CONVEX_WRONG = {"no_max_subtraction": dict(sub_max=False), "softmax_over_in_range_taps": dict(in_range_only=True), "ky_kx_swapped": dict(swap_ky_kx=True),
                "i_j_swapped": dict(swap_i_j=True), "replicate_padding": dict(pad="replicate"), "factor_4_missing": dict(factor=1.0)}
CONVEX3D_WRONG = dict(CONVEX_WRONG, kt_fastest=dict(kt_fastest=True), halo_frames_read_as_zero=dict(halo_zero=True),
                      one_frame_beyond_t_halo=dict(one_beyond=True))


@functools.lru_cache(maxsize=None)
def convex_inputs(dim, case, data):
    """flow (T + 2 t_halo, H, W, 2), mask (T, H, W, 144 or 432) fp32, t_halo (0 for the 2-D kernel)"""
    T, H, W = case[:3]
    th, ntap = (case[3], 27) if dim == 3 else (0, 9)
    seed = 9800 + 100 * dim + 10 * (CONVEX3D_CASES if dim == 3 else CONVEX2D_CASES).index(case) + CONVEX_DATA.index(data)
    flow = hash_normal((T + 2 * th, H, W, 2), seed) * (60.0 if data == "bigflow" else 3.0)
    mask = hash_normal((T, H, W, 16 * ntap), seed + 5)
    if data == "sharp":
        mask = (100.0 + 30.0 * mask).float()
    return flow.float(), mask, th


@functools.lru_cache(maxsize=None)
def convex_refs(dim, case, data):
    flow, mask, th = convex_inputs(dim, case, data)
    kt = 3 if dim == 3 else 1
    return convex_upsample_3d(flow, mask, th, kt=kt), convex_upsample_3d(flow, mask, th, kt=kt, dtype=torch.float32)


def convex_check(dim, case, data, out, label=None):
    ref, f32 = convex_refs(dim, case, data)
    return Check(label or f"convex_upsample{'_3d' if dim == 3 else ''} {case} {data}").add("out", out, ref, tol_reduce(ref, f32, False))


# ------------------------------------------------------------------------------------------------ tap gather-sum
TGS_HALO = 2
TGS_CASES = [  # cout, (kt, kh, kw), T, H, W, t_halo, y_ld, out_ld, accum_ld (None: no accum)
    (2, (3, 3, 3), 3, 5, 9, 0, 64, 4, 2),      # the engine's call (the unrolled kernel)
    (2, (3, 3, 3), 1, 1, 1, 0, 64, 4, 2),      # one pixel: 26 of the 27 taps outside
    (1, (1, 3, 3), 2, 4, 6, 0, 16, 3, None),   # the generic kernel, cout = 1, no accum
    (3, (3, 1, 3), 2, 5, 7, 1, 32, 4, 4),      # cout = 3, a halo frame on either side
    (2, (5, 1, 1), 4, 3, 5, 2, 16, 2, 3),      # kt = 5 reaches both halo frames; out_ld = cout
]


def tap_gather_sum(y, bias, cout, k3, T, H, W, t_halo, dtype=F64, order="kz_major", mirrored=False, column="tap_major", with_bias=True, halo_zero=False):
    """y ((T + 2 t_halo) H W, y_ld), bias (cout,) -> out (T H W, cout), and sum |terms| + |bias| of every element:
    out[p][c] = bias[c] + sum_tap y[p + d(tap)][tap cout + c], tap = (kz kh + ky) kw + kx, d(tap) = (kz - kt / 2, ky - kh / 2, kx - kw / 2), zero
    outside the frame and beyond the t_halo frames around the T own ones (loop_ops.hip).  dtype = float32: the plain-torch form.  The other
    keyword arguments are the wrong variants."""
    kt, kh, kw = k3
    ntap, Tf = kt * kh * kw, T + 2 * t_halo
    v = F.pad(y.to(dtype).reshape(Tf, H, W, -1), (0, 0, kw // 2, kw // 2, kh // 2, kh // 2, kt // 2, kt // 2))
    t = torch.arange(T)
    out = (bias.to(dtype) if with_bias else torch.zeros(cout, dtype=dtype)).reshape(1, 1, 1, cout).expand(T, H, W, cout).clone()
    mag = out.abs()
    for kz in range(kt):
        for ky in range(kh):
            for kx in range(kw):
                tap = (kz * kh + ky) * kw + kx if order == "kz_major" else (kx * kh + ky) * kt + kz
                cols = tap * cout + torch.arange(cout) if column == "tap_major" else torch.arange(cout) * ntap + tap
                dz, dy, dx = (kt // 2 - kz, kh // 2 - ky, kw // 2 - kx) if mirrored else (kz - kt // 2, ky - kh // 2, kx - kw // 2)
                tt = t + t_halo + dz                                        # frame of y
                ok = ((tt >= t_halo) & (tt < t_halo + T)) if halo_zero else ((tt >= 0) & (tt < Tf))
                term = v[(tt + kt // 2).clamp(0, Tf + 2 * (kt // 2) - 1), kh // 2 + dy:kh // 2 + dy + H, kw // 2 + dx:kw // 2 + dx + W][..., cols]
                term = torch.where(ok.reshape(T, 1, 1, 1), term, torch.zeros_like(term))
                out, mag = out + term, mag + term.abs()
    return out.reshape(T * H * W, cout), mag.reshape(T * H * W, cout)


def tap_gather_sum_f32(y, bias, cout, k3, T, H, W, t_halo):
    return tap_gather_sum(y, bias, cout, k3, T, H, W, t_halo, dtype=torch.float32)[0]


TGS_WRONG = {"kx_major_taps": dict(order="kx_major"), "taps_mirrored": dict(mirrored=True), "column_c_ntap+tap": dict(column="c_major"),
             "bias_dropped": dict(with_bias=False), "halo_frames_read_as_zero": dict(halo_zero=True), "accum_overwritten": None}      # None: accum = out, the out side is the reference's


@functools.lru_cache(maxsize=None)
def tgs_inputs(case):
    """y ((T + 2 t_halo) H W, ntap cout), bias (cout,), accum before the launch (T H W, cout) -- all fp32"""
    cout, k3, T, H, W, th = case[:6]
    seed = 9900 + 10 * TGS_CASES.index(case)
    ntap = k3[0] * k3[1] * k3[2]
    return hash_normal(((T + 2 * th) * H * W, ntap * cout), seed), hash_normal((cout,), seed + 1), hash_normal((T * H * W, cout), seed + 2) * 4


@functools.lru_cache(maxsize=None)
def tgs_ref(case):
    y, bias, _ = tgs_inputs(case)
    cout, k3, T, H, W, th = case[:6]
    return tap_gather_sum(y, bias, cout, k3, T, H, W, th)


def tgs_check(case, out, accum=None, label=None):
    """out (P, cout) within (ntap + 1) 2^-24 (|bias| + sum |terms|) of the reference: the first-order worst case of any-order fp32 summation
    of ntap + 1 terms; accum (P, cout) = fp32(accum before + out as returned), exact"""
    ref, mag = tgs_ref(case)
    ntap = case[1][0] * case[1][1] * case[1][2]
    bound = (ntap + 1) * 2.0 ** -24 * mag
    ck = Check(label or f"tap_gather_sum {case}").bound("out", out, ref, bound)
    got = out.detach().cpu().double()
    fine = got.shape == ref.shape and bool(torch.isfinite(got).all())
    ck.items.append(("out/bound", ((got - ref).abs() / bound).max().item() if fine else math.inf, 1.0))      # the same condition, as a ratio
    if case[8] is not None:
        ck.exact("accum", accum, tgs_inputs(case)[2] + out.detach().cpu().float())
    return ck


# ------------------------------------------------------------------------------------------------ bilinear resize
BILINEAR_CASES = [(2, 3, 5, 7, 10, 14), (1, 2, 6, 5, 9, 11), (1, 1, 4, 4, 4, 4), (1, 2, 9, 13, 3, 5), (1, 1, 3, 8, 1, 1), (1, 1, 1, 1, 4, 4),
                  (2, 1, 8, 32, 32, 128)]                                   # N, C, H, W, OH, OW: up, odd ratios, identity, down, one pixel out, one pixel in, 4 x
BILINEAR_MUL = (1.0, -0.5, 2.0)


def bilinear(x, OH, OW, align, mul):
    """x (N, C, H, W) -> mul F.interpolate(x, (OH, OW), "bilinear", align_corners) in float64"""
    return mul * F.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=bool(align))


def bilinear_f32(x, OH, OW, align, mul):
    return mul * F.interpolate(x.float(), size=(OH, OW), mode="bilinear", align_corners=bool(align))


def bilinear_taps(x, OH, OW, align, mul, clamp0=True, aligned_scale="(H-1)/(OH-1)"):
    """the same resize written out (aten/native/UpSample.h: area_pixel_compute_source_index), float64; the keyword arguments are wrong variants"""
    N, C, H, W = x.shape
    x = x.double()

    def axis(n, o):
        i = torch.arange(o, dtype=F64)
        if align:
            f = i * (((n - 1) / (o - 1) if o > 1 else 0.0) if aligned_scale == "(H-1)/(OH-1)" else n / o)
        else:
            f = (n / o) * (i + 0.5) - 0.5
            if clamp0:
                f = f.clamp_min(0.0)
        i0 = f.trunc().long().clamp(0, n - 1)                              # (int) f, as a kernel converts
        return i0, (i0 + 1).clamp_max(n - 1), f - i0
    y0, y1, ly = axis(H, OH)
    x0, x1, lx = axis(W, OW)
    ly, lx = ly.reshape(OH, 1), lx.reshape(1, OW)
    rows = lambda yy: x[:, :, yy][:, :, :, x0] * (1 - lx) + x[:, :, yy][:, :, :, x1] * lx
    return mul * (rows(y0) * (1 - ly) + rows(y1) * ly)


BILINEAR_WRONG = {
    "align_corners_exchanged": lambda x, OH, OW, al, mul: bilinear(x, OH, OW, not al, mul),
    "no_clamp_at_0": lambda x, OH, OW, al, mul: None if al else bilinear_taps(x, OH, OW, al, mul, clamp0=False),
    "nearest": lambda x, OH, OW, al, mul: mul * F.interpolate(x.double(), size=(OH, OW), mode="nearest"),
    "mul_dropped": lambda x, OH, OW, al, mul: bilinear(x, OH, OW, al, 1.0),
    "aligned_scale_H/OH": lambda x, OH, OW, al, mul: bilinear_taps(x, OH, OW, al, mul, aligned_scale="H/OH") if al else None,
}


@functools.lru_cache(maxsize=None)
def bilinear_input(case):
    N, C, H, W, OH, OW = case
    return hash_normal((N, C, H, W), 10000 + 10 * BILINEAR_CASES.index(case))


@functools.lru_cache(maxsize=None)
def bilinear_refs(case, align):
    """(reference, fp32 torch) at mul = 1: a mul of -0.5 or 2 scales both exactly"""
    x = bilinear_input(case)
    return bilinear(x, case[4], case[5], align, 1.0), bilinear_f32(x, case[4], case[5], align, 1.0)


def bilinear_check(case, align, mul, out, label=None):
    ref, f32 = bilinear_refs(case, align)
    return Check(label or f"bilinear {case} align={int(align)} mul={mul}").add("out", out, mul * ref, tol_reduce(mul * ref, mul * f32, False))


# ------------------------------------------------------------------------------------------------ tiled transposes
TRANSPOSE_CASES = [(2, 33, 65, 40), (1, 1, 31, 1), (3, 2, 45, 2), (1, 144, 60, 144), (1, 432, 35, 440), (2, 256, 33, 256)]      # BT, C, HW, ld
TRANSPOSE_F32_SRC_EXTRA = [(3, 2, 45, 4)]                                  # the engine's DFLOW read: 2 channels at ld 4
TRANSPOSE_SP_VIEW = (2, 33, 65, 48, 8)                                     # BT, C, HW, channels of the SP tensor, channel offset of the view


@functools.lru_cache(maxsize=None)
def transpose_input(BT, C, HW):
    """(BT, C, HW) fp32, all distinct, magnitudes spread evenly in the exponent over 2^-20 .. 2^20 and shuffled, alternating signs: neighbours
    in magnitude differ by 40 ln 2 / n > 2^-10 relative, so the values stay distinct as split bf16 holds them (16 significant bits)"""
    n = BT * C * HW
    g = torch.Generator().manual_seed(10100 + n)
    mag = torch.exp2(-20.0 + 40.0 * torch.randperm(n, generator=g).double() / n)
    return (mag * (1 - 2 * (torch.arange(n) % 2))).float().reshape(BT, C, HW)


def to_channel_last(x):
    """(BT, C, HW) -> (BT HW, C)"""
    return x.permute(0, 2, 1).reshape(-1, x.shape[1])


# ------------------------------------------------------------------------------------------------ device buffers of the GPU tests
GPU = "cuda:0"


def sp_out(L, pixels, channels):
    t = L.SPTensor(pixels, channels, GPU)
    t.data.fill_(SENTINEL)
    return t


def sp_in(L, values, extra=8, c0=0):
    """SP tensor whose channels [c0, c0 + C) hold `values` (P, C); the other channels hold the sentinel"""
    P, C = values.shape
    t = sp_out(L, P, c0 + C + extra)
    t.set_f32(values.to(GPU), c0)
    assert torch.equal(t.to_f32(c0, C).cpu(), values), "the reference must see what the kernel sees"
    return t


def sp_in_junk(L, values, channels, c0=0):
    """SP tensor of `channels` channels whose channels [c0, c0 + C) hold `values` (P, C); every other channel holds JUNK in both planes"""
    P, C = values.shape
    t = L.SPTensor(P, channels, GPU)
    t.data.fill_(JUNK)
    t.set_f32(values.to(GPU), c0)
    assert torch.equal(t.to_f32(c0, C).cpu(), values), "the reference must see what the kernel sees"
    return t


def f32_in(values, ld, misaligned=False):
    """(P, ld) fp32 device view holding `values` (P, C) with JUNK in the padding columns; misaligned: one float into its allocation"""
    P, C = values.shape
    off = 1 if misaligned else 0
    buf = torch.full((P * ld + 8,), JUNK, device=GPU)
    v = buf[off:off + P * ld].view(P, ld)
    v[:, :C] = values.to(GPU)
    assert v.data_ptr() % 16 == (4 if misaligned else 0)
    return v


def f32_out(n, tail=8):
    return torch.full((n + tail,), SENTINEL, device=GPU)


def planes_are(t, lo_c, hi_c, value):
    """both planes of channels [lo_c, hi_c) of the own pixels hold `value`"""
    return bool((t.own()[:, :, lo_c:hi_c].float() == value).all().item())


def report(ck):
    print(f"RATIO {ck.worst():.3f} | {ck}")
    assert ck.ok, str(ck)
