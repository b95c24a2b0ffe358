"""The fused activations of csrc/common.h (exp_fast, sigmoid_fast, tanh_fast, erf_fast, gelu_erf, apply_act_n) and the epilogue kinds of
csrc/conv_epilogue.h swept over their whole input range against float64: the value grid, its layout over (pixel, cout), the references,
the tolerance, an fp32 emulation of the formulas as common.h writes them (with its named wrong variants) and the launch builder that
tests/test_gpu_act_sweep.py drives.  tests/test_act_sweep_refs.py checks the pieces that need no GPU.

Isolating the activation.  The linear part of a launch is made exact, so that what is compared is the epilogue alone:
  identity injection  w[c, c % cin, centre tap] = 1, every other weight 0 (exact in bf16, lo plane zero), inputs with at most 16
                      significant bits (sp_round(x) == x): acc = hi + lo is exactly x[pix, c % cin] whatever the summation order;
  share injection     zero input, pre_f32[pix][c] = any fp32 value (the classes with pre_f32);
  bias injection      bias[c] = NaN / +-inf for single couts (the GEMM would spread a non-finite INPUT over its pixel and its neighbours).
What reaches the activation is v = fp32(injected + bias): the accumulator starts at +0, so an injected -0 arrives as +0 (pre_value()).
Every (kernel, shape) first runs ACT_NONE with scale 1 and must return pre_value() bit for bit; only then are the activations compared.

Reference: float64 torch on the CPU (act_ref, epi_ref).  Tolerance, per element: |got - ref| <= 2^-20 max(1, |pre-activation|, |aux|, |ref|).
tanh_fast is the worst form: 1 - 2 rcp(1 + exp2(2x log2e)) has two 1-ulp hardware operations and three fp32 roundings on values below 2;
to first order |d tanh| <= 2 r^2 (|d e| + ulp(1 + e)/2 + ...) + ulp(1)/2, about 4e-7 at its worst point (e ~ 0.05 .. 1).  2^-20 = 9.5e-7 is
the next power of two that leaves a factor of two over it, five times the emulation's own 1.9e-7 and fifty times below the 5e-5 of the
conv tests.  ACT_NONE, ACT_RELU, scale = 0.25 and every non-finite pre-activation are compared exactly.

Left out on purpose: gelu(-inf) (it is -inf * 0), and +-inf through SP outputs (split_bf16(inf) has lo = inf - inf = NaN by construction)."""
import math

import numpy as np
import torch

import kernel_refs as R
from ppmstereo_amd import _lib as L
from ppmstereo_amd.weights import hash_normal

F64 = torch.float64
TOL = 2.0 ** -20
SENT = 24576.0                                                             # fills every output before a launch: exact in bf16, and no activation of the grid gives it
NAN, INF = float("nan"), float("inf")
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.ACT_SIGMOID, L.ACT_TANH, L.ACT_ELU1)
ACT_NAMES = {L.ACT_NONE: "none", L.ACT_RELU: "relu", L.ACT_GELU: "gelu", L.ACT_SIGMOID: "sigmoid", L.ACT_TANH: "tanh", L.ACT_ELU1: "elu1"}
KIND_NAMES = {L.EPI_STORE: "store", L.EPI_RESID: "resid", L.EPI_RH: "rh", L.EPI_GRU: "gru"}


# ------------------------------------------------------------------------------------------------ the value grid
def _ulps(center: float, n: int) -> torch.Tensor:
    """the 2 n + 1 fp32 values within n ulps of (positive) `center`"""
    c = torch.tensor([center], dtype=torch.float32).view(torch.int32)
    return (c + torch.arange(-n, n + 1, dtype=torch.int32)).view(torch.float32)


_LN2 = math.log(2.0)
# where exp_fast's exp2 argument crosses 128 (overflow), -126 (first denormal result) and -149 / -150 (zero), and the same for tanh's 2x
EXP_POINTS = (128 * _LN2, 126 * _LN2, 149 * _LN2, 150 * _LN2, 64 * _LN2, 63 * _LN2)
EXP_SPANS = ((44.0, 44.5), (87.0, 89.0), (103.0, 104.5))
GRID_N = 5749                                                              # <= 120 pixels x 51 couts, the smallest launch (SMALLEST)


def _build_grid(bits: int) -> torch.Tensor:
    k = torch.arange(1, 33, dtype=F64)
    near = _ulps(0.125, 32) if bits == 32 else torch.cat([0.125 - k.flip(0) * 2.0 ** -19, torch.tensor([0.125], dtype=F64), 0.125 + k * 2.0 ** -18]).float()
    mags = [torch.logspace(-20, math.log2(110.0), 2048, base=2.0, dtype=F64).float(),      # 2^-20 .. 110
            near]                                                                          # +-32 steps around the branch point of tanh_fast
    mags += [torch.linspace(a, b, 32, dtype=F64).float() for a, b in EXP_SPANS]
    mags += [_ulps(p, 2) for p in EXP_POINTS]
    mags += [torch.tensor([1e20, 1e30]), torch.logspace(7, 127, 64, base=2.0, dtype=F64).float()]      # huge finite values, up to 2^127
    m = torch.cat(mags)
    fixed = torch.cat([torch.tensor([0.0, -0.0]), m, -m])
    fill = torch.linspace(-8.0, 8.0, GRID_N - fixed.numel(), dtype=F64).float()            # the uniform fill of [-8, 8]
    g = torch.cat([fixed, fill])
    assert g.numel() == GRID_N
    return g


GRID32 = _build_grid(32)                                                   # full fp32 spacing: the share and bias injections
GRID16 = R.sp_round(_build_grid(16))                                       # what a split-bf16 input holds exactly: the identity injection; its
#                                                                            neighbourhood of 0.125 is +-32 steps of 16-bit spacing (2^-19 below, 2^-18 above)
PERM = torch.argsort(hash_normal((GRID_N,), 9001))                         # position i of a layout holds grid[PERM[i % GRID_N]]: fixed, seeded

RANGES = {  # name -> [lo, hi) of |x|: what every 8-cout group of a layout must see
    "tiny": (0.0, 2.0 ** -10), "small": (2.0 ** -10, 0.1249), "branch": (0.1249, 0.1252), "mid": (0.1252, 8.0), "tail": (8.0, 44.0),
    "edge44": (44.0, 44.5001), "far": (44.5001, 87.0), "edge88": (87.0, 89.0001), "edge103": (103.0, 104.5001), "beyond": (104.5001, INF),
}


def layout(grid: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """(rows, cols) of grid values under the fixed permutation; rows * cols >= GRID_N places every grid value at least once"""
    i = torch.arange(rows * cols, dtype=torch.int64)
    return grid[PERM[i % GRID_N]].reshape(rows, cols).clone()


def special_couts(n_valid: int) -> dict:
    """the couts that receive a non-finite bias: NaN in the LAST valid cout (inside the ragged 4-wide tail where there is one), +-inf in two
    different 8-cout rows; their neighbours prove they stay untouched"""
    return {"nan": n_valid - 1, "+inf": 2, "-inf": 11}


def grid_cols(n: int, n_valid: int) -> list:
    """the columns of an n-wide injection that carry grid values: those a cout reads, less the special couts (they hold 0 and get their
    value from the bias)"""
    sp = set(special_couts(n_valid).values())
    return [c for c in range(min(n, n_valid)) if c not in sp]


def injection(grid: torch.Tensor, P: int, n: int, n_valid: int) -> torch.Tensor:
    """(P, n) fp32: the grid laid over the pixels and the non-special columns"""
    cols = grid_cols(n, n_valid)
    x = torch.zeros(P, n)
    x[:, cols] = layout(grid, P, len(cols))
    return x


def special_bias(n_valid: int, act: int, kind: int) -> torch.Tensor:
    """(n_valid,) fp32 bias: NaN at its cout for every launch; +-inf only where the result is defined and exact: STORE with NONE, RELU,
    SIGMOID or TANH (not GELU: -inf * 0; not ELU1 / the aux kinds: kept to the tolerance-free cases)"""
    b = torch.zeros(n_valid)
    sp = special_couts(n_valid)
    b[sp["nan"]] = NAN
    if kind == L.EPI_STORE and act in (L.ACT_NONE, L.ACT_RELU, L.ACT_SIGMOID, L.ACT_TANH):
        b[sp["+inf"]], b[sp["-inf"]] = INF, -INF
    return b


def pre_value(inj: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """what the activation sees, in fp32 as the kernels compute it: (acc = injected value, from +0) + bias; -0 arrives as +0"""
    return (inj.float() + 0.0) + bias.float()


def aux_values(P: int, n: int) -> torch.Tensor:
    """the SP state operand of RESID / RH / GRU: 16-bit values of a few units, both signs, zero included"""
    a = R.sp_round(torch.linspace(-3.0, 3.0, 1021, dtype=F64).float()[(torch.arange(P * n) * 389) % 1021].reshape(P, n))
    a[0, 0] = 0.0
    return a


def gate_values(P: int, n: int) -> torch.Tensor:
    """the fp32 update gate z of the GRU epilogue: [0, 1] with both ends"""
    return torch.linspace(0.0, 1.0, 509, dtype=F64).float()[(torch.arange(P * n) * 211) % 509].reshape(P, n).clone()


# ------------------------------------------------------------------------------------------------ float64 references
def act_ref(act: int, x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    if act == L.ACT_RELU:
        return torch.where(x < 0, torch.zeros_like(x), x)                   # NaN stays NaN
    if act == L.ACT_GELU:
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))            # = 0.5 x (1 + erf(x / sqrt 2)) without the cancellation
    if act == L.ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-x))
    if act == L.ACT_TANH:
        return torch.tanh(x)
    if act == L.ACT_ELU1:
        return torch.where(x > 0, x + 1.0, torch.exp(x))
    return x


def pre_activation(kind: int, v: torch.Tensor, aux=None) -> torch.Tensor:
    """fp32 argument of the activation: v, or aux + v rounded as the kernel rounds it (RESID)"""
    return (aux.float() + v.float()) if kind == L.EPI_RESID else v.float()


def epi_ref(kind: int, act: int, scale: float, v: torch.Tensor, aux=None, z=None) -> torch.Tensor:
    """float64 result of one epilogue on fp32 pre-activations v"""
    v = v.double()
    if kind == L.EPI_STORE:
        return act_ref(act, v) * scale
    if kind == L.EPI_RESID:
        return act_ref(act, aux.double() + v) * scale
    if kind == L.EPI_RH:
        return act_ref(L.ACT_SIGMOID, v) * aux.double()
    assert kind == L.EPI_GRU
    return (1.0 - z.double()) * aux.double() + z.double() * torch.tanh(v)


def is_exact(kind: int, act: int) -> bool:
    """no transcendental, one rounding at most, and that one reproduced in fp32 by the reference: compared bit for bit"""
    return kind in (L.EPI_STORE, L.EPI_RESID) and act in (L.ACT_NONE, L.ACT_RELU)


def exact_ref(kind: int, act: int, scale: float, v: torch.Tensor, aux=None) -> torch.Tensor:
    """fp32 result of the exact cases (scale a power of two)"""
    x = pre_activation(kind, v, aux)
    if act == L.ACT_RELU:
        x = torch.where(x < 0, torch.zeros_like(x), x)
    return x * scale


def tolerance(pre: torch.Tensor, ref: torch.Tensor, aux=None) -> torch.Tensor:
    t = torch.maximum(pre.double().abs(), ref.double().abs()).clamp_min(1.0)
    if aux is not None:
        t = torch.maximum(t, aux.double().abs())
    return TOL * t


class Outcome:
    """one comparison: .bad elements over the bound (or not bit-equal where exactness is asked); .ratio the largest error / bound over the
    finite elements, found at pre-activation .x with |got - ref| = .err"""

    def __init__(self, label, bad, err, x, ratio, first):
        self.label, self.bad, self.err, self.x, self.ratio, self.first = label, bad, err, x, ratio, first

    @property
    def ok(self):
        return self.bad == 0

    def __str__(self):
        return f"{self.label}: {self.bad} bad, worst {self.ratio:.3f} of the bound: err {self.err:.3e} at x = {self.x!r}" + (f"; first bad: {self.first}" if self.first else "")


def same_bits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """elementwise: equal bit for bit, any NaN equal to any NaN"""
    a, b = a.float().contiguous(), b.float().contiguous()
    return (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))


def compare(label: str, kind: int, act: int, scale: float, got: torch.Tensor, v: torch.Tensor, aux=None, z=None, scale_bound: float = 1.0) -> Outcome:
    """got (fp32, CPU) against the reference of fp32 pre-activations v.  Exact cases and non-finite pre-activations: bit for bit; everything
    else: the per-element bound, times scale_bound (the CPU test asks the emulation for half of it)."""
    got = got.detach().cpu().float()
    pre = pre_activation(kind, v, aux)
    ref = epi_ref(kind, act, scale, v, aux, z)
    special = ~torch.isfinite(pre)
    if is_exact(kind, act) or scale != 1.0:
        assert is_exact(kind, act), "a scale is only swept with the exact activations"
        okm = same_bits(got, exact_ref(kind, act, scale, v, aux))
        err = torch.zeros_like(ref)
        tol = torch.ones_like(ref)
    else:
        tol = tolerance(pre, ref, aux if kind != L.EPI_STORE else None) * scale_bound
        err = (got.double() - ref).abs()
        okm = torch.where(special, same_bits(got, ref.float()), torch.isfinite(got) & (err <= tol))
        err = torch.where(special | ~torch.isfinite(err), torch.zeros_like(err), err)
    bad = int((~okm).sum())
    first = None
    if bad:
        i = int((~okm).flatten().nonzero()[0])
        first = f"[{i // got.shape[1]}, {i % got.shape[1]}] x = {pre.flatten()[i].item()!r} got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r}"
    rel = torch.where(torch.isfinite(tol), err / tol, torch.zeros_like(err))
    j = int(rel.flatten().argmax())
    return Outcome(label, bad, err.flatten()[j].item(), pre.flatten()[j].item(), rel.flatten()[j].item(), first)


# ------------------------------------------------------------------------------------------------ fp32 emulation of common.h
f32 = np.float32


def _exp2(x):
    """correctly rounded fp32 exp2 (float64 exp2, rounded once)"""
    return np.exp2(x.astype(np.float64)).astype(f32)


def _rcp(x):
    return (1.0 / x.astype(np.float64)).astype(f32)


class Emulation:
    """The formulas of common.h / conv_epilogue.h in fp32 numpy, operation by operation, with exp2 and the reciprocal correctly rounded
    (the hardware's are 1 ulp).  The keyword arguments are the named wrong variants that the sweep must reject."""

    def __init__(self, gelu="erf", erf="7.1.26", tanh_x5=True, tanh_branch=0.125, sigmoid_clamp=None, relu="select", gru_swapped=False, rh="sigmoid"):
        self.gelu_form, self.erf_fit, self.tanh_x5, self.tanh_branch = gelu, erf, tanh_x5, f32(tanh_branch)
        self.sigmoid_clamp, self.relu_form, self.gru_swapped, self.rh_gate = sigmoid_clamp, relu, gru_swapped, rh

    def exp_fast(self, x):
        return _exp2(x * f32(1.4426950408889634))

    def sigmoid(self, x):
        if self.sigmoid_clamp is not None:
            x = np.clip(x, f32(-self.sigmoid_clamp), f32(self.sigmoid_clamp))
        return _rcp(f32(1.0) + self.exp_fast(-x))

    def tanh(self, x):
        big = f32(1.0) - f32(2.0) * _rcp(f32(1.0) + self.exp_fast(f32(2.0) * x))
        x2 = x * x
        c5 = f32(0.13333333333) if self.tanh_x5 else f32(0.0)
        small = x * (f32(1.0) + x2 * (f32(-0.33333333333) + x2 * (c5 - f32(0.05396825397) * x2)))
        return np.where(np.abs(x) < self.tanh_branch, small, big)

    def erf(self, x):
        ax = np.abs(x)
        if self.erf_fit == "7.1.26":
            t = _rcp(f32(1.0) + f32(0.3275911) * ax)
            poly = t * (f32(0.254829592) + t * (f32(-0.284496736) + t * (f32(1.421413741) + t * (f32(-1.453152027) + t * f32(1.061405429)))))
        else:                                                               # Abramowitz & Stegun 7.1.25: three terms, |error| <= 2.5e-5
            t = _rcp(f32(1.0) + f32(0.47047) * ax)
            poly = t * (f32(0.3480242) + t * (f32(-0.0958798) + t * f32(0.7478556)))
        y = f32(1.0) - poly * self.exp_fast(-ax * ax)
        return np.copysign(y, x)

    def gelu(self, x):
        if self.gelu_form == "tanh":
            return f32(0.5) * x * (f32(1.0) + self.tanh(f32(0.7978845608) * (x + f32(0.044715) * x * x * x)))
        return f32(0.5) * x * (f32(1.0) + self.erf(x * f32(0.70710678118654752440)))

    def act(self, act, x):
        if act == L.ACT_RELU:
            return np.fmax(x, f32(0.0)) if self.relu_form == "fmax" else np.where(x < f32(0.0), f32(0.0), x)
        if act == L.ACT_GELU:
            return self.gelu(x)
        if act == L.ACT_SIGMOID:
            return self.sigmoid(x)
        if act == L.ACT_TANH:
            return self.tanh(x)
        if act == L.ACT_ELU1:
            return np.where(x > f32(0.0), x + f32(1.0), np.exp(x.astype(np.float64)).astype(f32))       # (expf: the library's, correctly rounded here)
        return x

    def epilogue(self, kind, act, scale, v, aux=None, z=None) -> torch.Tensor:
        """fp32 torch result of one epilogue on fp32 torch operands"""
        n = lambda t: None if t is None else t.float().numpy().astype(f32)
        v, aux, z = n(v), n(aux), n(z)
        with np.errstate(all="ignore"):
            if kind == L.EPI_STORE:
                y = self.act(act, v) * f32(scale)
            elif kind == L.EPI_RESID:
                y = self.act(act, aux + v) * f32(scale)
            elif kind == L.EPI_RH:
                y = (self.tanh(v) if self.rh_gate == "tanh" else self.sigmoid(v)) * aux
            else:
                th = self.tanh(v)
                y = z * aux + (f32(1.0) - z) * th if self.gru_swapped else (f32(1.0) - z) * aux + z * th
        return torch.from_numpy(np.ascontiguousarray(y, dtype=f32))


WRONG = {  # name -> (Emulation arguments, (kind, act) of the launch that must reject it)
    "gelu_tanh_form": (dict(gelu="tanh"), (L.EPI_STORE, L.ACT_GELU)),
    "erf_7.1.25": (dict(erf="7.1.25"), (L.EPI_STORE, L.ACT_GELU)),
    "tanh_x5_dropped": (dict(tanh_x5=False), (L.EPI_STORE, L.ACT_TANH)),
    "tanh_branch_0.5": (dict(tanh_branch=0.5), (L.EPI_STORE, L.ACT_TANH)),
    "sigmoid_clamped_10": (dict(sigmoid_clamp=10.0), (L.EPI_STORE, L.ACT_SIGMOID)),
    "relu_fmax": (dict(relu="fmax"), (L.EPI_STORE, L.ACT_RELU)),
    "gru_z_swapped": (dict(gru_swapped=True), (L.EPI_GRU, L.ACT_NONE)),
    "rh_tanh": (dict(rh="tanh"), (L.EPI_RH, L.ACT_NONE)),
}

# every (kind, act) a launch of the sweep runs
EPI_CASES = [(L.EPI_STORE, a) for a in ACTS] + [(L.EPI_RESID, L.ACT_GELU), (L.EPI_RESID, L.ACT_RELU), (L.EPI_RH, L.ACT_NONE), (L.EPI_GRU, L.ACT_NONE)]
SMALLEST = (2 * 6 * 10, 54)                                                # pixels and valid couts of the smallest launch (conv_gemm2 64 -> 54)


def cpu_case(kind: int, act: int, grid: torch.Tensor = None, P: int = SMALLEST[0], n_valid: int = SMALLEST[1]):
    """(v, aux, z) of one launch as the GPU test builds them, on the CPU"""
    grid = GRID16 if grid is None else grid
    v = pre_value(injection(grid, P, n_valid, n_valid), special_bias(n_valid, act, kind))
    return v, aux_values(P, n_valid), gate_values(P, n_valid)


# ------------------------------------------------------------------------------------------------ V^T encoding
def vt_bits(y: torch.Tensor, vt_f16: int) -> torch.Tensor:
    """int16 bits of vt_enc(y) (common.h) for fp32 y, in torch: bf16(y), or the fp16 number equal to it saturated at +-65504 (NaN passes)"""
    b = y.float().to(torch.bfloat16)
    if not vt_f16:
        return b.view(torch.int16)
    v = b.float()
    v = torch.where(v > 65504.0, torch.full_like(v, 65504.0), torch.where(v < -65504.0, torch.full_like(v, -65504.0), v))
    return v.to(torch.float16).view(torch.int16)


VT_VALUES = (65504.0, -65504.0, 65520.0, -65520.0, 1e5, -1e5, 65280.0, -65280.0, 2.0 ** -14, 2.0 ** -20, -(2.0 ** -24))      # + NaN through the bias


# ------------------------------------------------------------------------------------------------ launches (GPU)
GPU = "cuda:0"
GUARD = 64                                                                 # sentinel elements before and after every output


class Half:
    """one epilogue half of a launch: what it computes and which outputs it writes"""

    def __init__(self, n_valid, kind=L.EPI_STORE, act=L.ACT_NONE, scale=1.0, pre=False, sp=True, f32=True, vt=None):
        self.n_valid, self.kind, self.act, self.scale, self.pre, self.sp, self.f32, self.vt = n_valid, kind, act, scale, pre, sp, f32, vt


class Kernel:
    """a conv kernel form: ConvOp version, hint (conv_gemm2's wm, conv_gemm5's blocks per tile), y-swept form, K slices, padded rows"""

    def __init__(self, name, version, hint=0, ysweep=False, nslice=None, m_pad=None):
        self.name, self.version, self.hint, self.ysweep, self.nslice, self.m_pad = name, version, hint, ysweep, nslice, m_pad

    def __repr__(self):
        return self.name


class Site:
    """One (kernel, shape, cin -> couts, taps): the identity weights, packed once per bias, and the inputs, uploaded once; run() launches
    one epilogue configuration twice into sentinel-filled outputs and returns them with the fp32 pre-activations the reference needs."""

    def __init__(self, kernel: Kernel, T, H, W, cin, couts, k3, m_split=None, cout_map=None, extra=()):
        from ppmstereo_amd.convplan import CONV2_SWEPT
        self.kernel, self.T, self.H, self.W, self.cin, self.couts, self.k3 = kernel, T, H, W, cin, list(couts), k3
        self.P, self.HW = T * H * W, H * W
        self.m_split, self.cout_map = m_split, cout_map
        self.key = CONV2_SWEPT if kernel.ysweep else kernel.version
        rows = sum(self.couts)
        w = torch.zeros(rows, cin, *k3)
        r = torch.arange(rows)
        w[r, r % cin, k3[0] // 2, k3[1] // 2, k3[2] // 2] = 1.0
        self.w = w
        self.x16 = injection(GRID16, self.P, cin, min(self.couts))           # identity injection: the special couts' channels stay 0
        if len(extra):                                                       # (the V^T sites: values around fp16's largest finite number)
            self.x16[1, 16:16 + len(extra)] = torch.tensor(extra)
        assert torch.equal(R.sp_round(self.x16), self.x16), "identity injection needs values a split-bf16 pair holds exactly"
        self.xin, self.packs = {}, {}

    def grid_fits(self) -> bool:
        """every grid value reaches a cout: through the identity injection, and through a share injection of the narrowest half"""
        n = min(self.couts)
        return self.P * len(grid_cols(self.cin, n)) >= GRID_N and self.P * len(grid_cols(n, n)) >= GRID_N

    def _input(self, zero: bool):
        """the SP input segment: the 16-bit grid, or zeros (share injection)"""
        if zero not in self.xin:
            t = L.SPTensor(self.P, self.cin, GPU)
            if not zero:
                t.set_f32(self.x16.to(GPU))
                assert torch.equal(t.to_f32().cpu(), self.x16)
            self.xin[zero] = t
        return self.xin[zero]

    def _pack(self, bias: torch.Tensor):
        from ppmstereo_amd.convplan import pack_for
        key = bias.numpy().tobytes()
        if key not in self.packs:
            self.packs[key] = pack_for(self.key, self.w.to(GPU), bias.to(GPU), [self.cin], None, self.cout_map, self.kernel.m_pad)
        return self.packs[key]

    def injected(self, h: int, half: Half) -> torch.Tensor:
        """(P, n_valid) fp32 values injected into half h, before the bias"""
        if half.pre:
            return injection(GRID32, self.P, half.n_valid, half.n_valid)
        r0 = sum(self.couts[:h])
        return self.x16[:, (torch.arange(half.n_valid) + r0) % self.cin]

    def run(self, halves):
        """launch twice; -> per half a dict: v (fp32 pre-activation, before aux), aux, z, f32, hi, lo, vt (CPU tensors), intact (everything
        around the outputs still holds the sentinel), same (the second launch gave the same bits)"""
        from ppmstereo_amd.convplan import ConvOp, conv_desc, epilogue
        k, P = self.kernel, self.P
        assert len(halves) == len(self.couts) and all(hf.n_valid == c for hf, c in zip(halves, self.couts))
        share = any(hf.pre for hf in halves)
        assert all(hf.pre for hf in halves) or not share, "one injection per launch"
        bias = torch.cat([special_bias(hf.n_valid, hf.act, hf.kind) for hf in halves])
        packed, b, meta = self._pack(bias)
        keep, epis, outs = [packed, b], [], []
        for h, hf in enumerate(halves):
            n = hf.n_valid
            ld = (n + 7) // 8 * 8 + 8
            o = dict(half=hf, ld=ld, bufs=[])
            kw = dict(kind=hf.kind, act=hf.act, scale=hf.scale, n_valid=n)
            if hf.sp:
                o["sp"] = L.SPTensor(P, ld, GPU, before=1, after=1)
                kw["out_sp"] = o["sp"].view(0, n)
                o["bufs"].append(o["sp"].data)
            if hf.f32:
                o["f32buf"] = torch.empty(P * ld + 2 * GUARD, device=GPU)
                o["f32view"] = o["f32buf"][GUARD:GUARD + P * ld].view(P, ld)
                kw.update(out_f32=o["f32view"], out_f32_ld=ld)
                o["bufs"].append(o["f32buf"])
            if hf.vt is not None:
                o["vtbuf"] = torch.empty(P * n + 2 * GUARD, dtype=torch.bfloat16, device=GPU)
                o["vtview"] = o["vtbuf"][GUARD:GUARD + P * n].view(self.T, n, self.HW)
                kw.update(out_vt=o["vtview"], vt_f16=hf.vt)
                o["bufs"].append(o["vtbuf"])
            if hf.kind in (L.EPI_RESID, L.EPI_RH, L.EPI_GRU):
                at = R.sp_in_junk(L, aux_values(P, n), ld)
                kw["aux_sp"] = at.view(0, n)
                o["aux"] = at.to_f32(0, n).cpu()
                keep.append(at)
            if hf.kind == L.EPI_GRU:
                o["z"] = gate_values(P, n)
                zt = R.f32_in(o["z"], ld)
                kw.update(aux_f32=zt, aux_f32_ld=ld)
                keep.append(zt)
            inj = self.injected(h, hf)
            if hf.pre:
                pt = R.f32_in(inj, ld)
                kw.update(pre_f32=pt)
                keep.append(pt)
            r0 = sum(self.couts[:h])
            o["v"] = pre_value(inj, bias[r0:r0 + n])
            epis.append(epilogue(**kw))
            outs.append(o)
        xin = self._input(share)
        d = conv_desc([xin.view()], (self.T, self.H, self.W), self.k3, epis[0], epis[1] if len(epis) > 1 else None, self.m_split or 0)
        d.w, d.bias, d.M = packed.data_ptr(), b.data_ptr(), meta["M"]
        if d.m_split == 0:
            d.m_split = meta["M"]
        bufs = [t for o in outs for t in o["bufs"]]
        op = ConvOp(d, keep + [xin] + bufs, k.version, k.hint, nslice=k.nslice if k.nslice is not None else 1, ysweep=k.ysweep)
        assert k.nslice is None or op.nslice == k.nslice
        bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        first = None
        for _ in range(2):
            for t in bufs:
                t.fill_(SENT)
            op()
            torch.cuda.synchronize()
            if first is None:
                first = [bits(t).clone() for t in bufs]
        same = all(torch.equal(a, bits(t)) for a, t in zip(first, bufs))
        for o in outs:
            n = o["half"].n_valid
            intact = True
            if "sp" in o:
                t = o["sp"]
                o["hi"], o["lo"] = t.own()[0, :, :n].cpu(), t.own()[1, :, :n].cpu()
                intact &= bool((t.own()[:, :, n:].float() == SENT).all()) and bool((t.data[:, :1].float() == SENT).all()) and bool((t.data[:, -1:].float() == SENT).all())
            if "f32buf" in o:
                o["f32"] = o["f32view"][:, :n].cpu()
                intact &= bool((o["f32view"][:, n:] == SENT).all()) and bool((o["f32buf"][:GUARD] == SENT).all()) and bool((o["f32buf"][-GUARD:] == SENT).all())
            if "vtbuf" in o:
                o["vt"] = o["vtview"].cpu()
                intact &= bool((o["vtbuf"][:GUARD].float() == SENT).all()) and bool((o["vtbuf"][-GUARD:].float() == SENT).all())
            o["intact"], o["same"] = intact, same
        return outs


def _sites():
    from ppmstereo_amd.packing import CONV2, CONV5, CONV6, GEMM1, STREAM
    s = {}
    for wm in (0, 1):                                                       # conv_gemm2: the shapes of test_conv_gemm_epilogues; 54: the ragged 4-wide tail
        for co in (64, 54):
            s[f"conv_gemm2-wm{wm}-{co}"] = (Kernel(f"conv_gemm2 wm={wm}", CONV2, wm), 2, 6, 10, 64, [co], (1, 3, 3))
    s["conv_gemm2-yswept-64"] = (Kernel("conv_gemm2 y-swept", CONV2, ysweep=True), 2, 6, 10, 64, [64], (1, 5, 1))
    s["conv_gemm2-sliced-190"] = (Kernel("conv_gemm2 K-sliced + reduce", CONV2, nslice=2), 4, 7, 9, 128, [190], (3, 3, 3))     # test_conv_gemm_k_sliced "3x3x3"
    s["conv_stream-64"] = (Kernel("conv_stream", STREAM), 2, 6, 10, 64, [64], (1, 3, 3))
    s["conv_stream-128"] = (Kernel("conv_stream", STREAM), 2, 6, 24, 128, [128], (1, 1, 5))
    for px in (7, 8):
        for co in (128, 256, 190):
            s[f"conv_gemm5-{px}-{co}"] = (Kernel(f"conv_gemm5 {px} blocks", CONV5, px), 2, 12, 64, 64, [co], (1, 3, 3))
    for co, m in ((128, 128), (256, 256), (190, 192)):
        s[f"conv_gemm6-{co}"] = (Kernel("conv_gemm6", CONV6, m_pad=m), 2, 12, 64, 64, [co], (1, 3, 3))
    s["gemm1-128"] = (Kernel("gemm1", GEMM1), 2, 8, 32, 128, [128], (1, 1, 1))
    s["gemm1-54"] = (Kernel("gemm1", GEMM1), 3, 5, 40, 256, [54], (1, 1, 1))
    return s


SITES = _sites()                                                           # id -> Site arguments: one full sweep of the epilogue classes each


def site(sid: str) -> Site:
    return Site(*SITES[sid])


def smallest_launches():
    """(pixels, input channels, valid couts) of every site: the grid must fit each"""
    return {sid: (a[1] * a[2] * a[3], a[4], min(a[5])) for sid, a in SITES.items()}


def refusal(fn) -> str:
    """the library's message when fn() is refused ("" when it is not)"""
    try:
        fn()
    except RuntimeError as e:
        return str(e)
    return ""


# ------------------------------------------------------------------------------------------------ the same functions outside the convs
def storage_bound(ref: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """split-bf16 outputs of an activation: the storage's 2^-16 |ref| on top of the activation's 2^-20 max(1, |x|), per element"""
    return ref.double().abs() * 2.0 ** -16 + TOL * x.double().abs().clamp_min(1.0)


DWG_SWEEP = {7: (3, 8, 16, 64, 72), 1: (1, 9, 17, 40, 64)}                  # k -> BT, H, W, channels, ld: kernel_refs.DWG_CASES "full64" and "view40_k1"


def dwg_sweep_input(k: int) -> torch.Tensor:
    """(BT, H, W, c) of the 16-bit grid: with zero depthwise weights and bias ppms_dwconv_gelu returns gelu(x) of it"""
    BT, H, W, c, _ = DWG_SWEEP[k]
    assert BT * H * W * c >= GRID_N
    return layout(GRID16, BT * H * W, c).reshape(BT, H, W, c)


# convex upsampling (ppms_convex_upsample / _3d): the softmax over 9 / 27 taps that writes the model's output
CONVEX_LOGITS = ("normal_x30", "one_tap_+80", "all_equal", "one_tap_-1e4")
CONVEX_2D = [(2, 6, 10), (2, 1, 7), (2, 6, 1)]                              # BT, H, W
CONVEX_3D = [(2, 5, 9, 0), (2, 5, 9, 1), (2, 1, 4, 1), (2, 4, 1, 1)]        # T, H, W, t_halo


def convex_logits(case: str, P: int, taps: int, seed: int) -> torch.Tensor:
    """(P, taps * 16) fp32 logits, channel 16 k + 4 i + j"""
    m = hash_normal((P, taps, 16), seed)
    if case == "normal_x30":
        m = m * 30.0
    elif case == "all_equal":
        m = hash_normal((P, 1, 16), seed + 1).expand(P, taps, 16).clone()
    else:
        k = (torch.arange(P * 16) * 7 % taps).reshape(P, 1, 16)
        m.scatter_(1, k, m.gather(1, k) + 80.0 if case == "one_tap_+80" else torch.full((P, 1, 16), -1e4))
    return m.reshape(P, taps * 16).contiguous()


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor, t_halo: int = 0, dtype=F64) -> torch.Tensor:
    """flow (T + 2 t_halo, H, W, 2), mask (T, H, W, taps * 16), taps 9 (2-D: t_halo 0) or 27 -> (T, 2, 4 H, 4 W), tap by tap:
    out[t, c, 4y+i, 4x+j] = sum_k softmax_k(mask[t, y, x, 16k + 4i + j]) * 4 flow[t + kt - 1, y + ky - 1, x + kx - 1, c], k = (kt 3 + ky) 3 + kx,
    zero outside the map and outside the frames the flow holds (loop_ops.hip).  dtype float32: the same in plain fp32 torch."""
    T, H, W, ch = mask.shape
    taps = ch // 16
    w = torch.softmax(mask.to(dtype).reshape(T, H, W, taps, 4, 4), 3)
    fl = 4.0 * flow.to(dtype)
    out = torch.zeros(T, 2, H, 4, W, 4, dtype=dtype)
    for k in range(taps):
        dt, dy, dx = (k // 9 - 1 if taps == 27 else 0), (k // 3) % 3 - 1, k % 3 - 1
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y0 >= y1 or x0 >= x1:
            continue
        for t in range(T):
            tt = t + dt + t_halo
            if 0 <= tt < fl.shape[0]:
                nb = fl[tt, y0 + dy:y1 + dy, x0 + dx:x1 + dx]                 # (h, w, 2)
                out[t, :, y0:y1, :, x0:x1, :] += torch.einsum("yxij,yxc->cyixj", w[t, y0:y1, x0:x1, k], nb)
    return out.reshape(T, 2, 4 * H, 4 * W)
