"""Plain float64 CPU references of the non-convolution kernels of the two encoders (encoder_ops.hip) and of the glue kernels around the
loop (small_ops.hip), one function per operation, each with the named wrong variants its test exists to catch; the cases (shapes and
seeded inputs) of tests/test_gpu_encoder_ops.py and tests/test_gpu_glue_ops.py; and the tolerance rule both they and the CPU test
tests/test_kernel_refs.py apply.  The formulas are those of oracle/ppm_oracle.py and of the kernel comments.

Tolerances, three kinds, none taken from the code under test:
 (a) exact: copies, permutations, the relu half, flow_add, the hi plane of any split (Check.exact);
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
