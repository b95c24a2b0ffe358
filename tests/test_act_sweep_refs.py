"""CPU: what keeps tests/test_gpu_act_sweep.py honest.  The fp32 emulation of common.h's formulas must pass the sweep's own check with half
the bound on the whole grid and for every epilogue kind (so the documented algorithm passes with margin); each named wrong variant must
fail that check on the same grid; and the grid must be what its docstring says: SP-exact in its 16-bit form, small enough for the smallest
launch of every kernel, and every range of it present in every 8-cout group and every 32-pixel tile of the layout."""
import math

import pytest
import torch
import torch.nn.functional as F

import act_sweep as S
from ppmstereo_amd import _lib as L

CASE_IDS = [f"{S.KIND_NAMES[k]}-{S.ACT_NAMES[a]}" for k, a in S.EPI_CASES]


# ------------------------------------------------------------------------------------------------ the references themselves
def test_references_are_the_plain_functions():
    """act_ref against torch's own float64 functions where they do not cancel (|x| <= 8), and the GELU tail against the erfc form's limit"""
    x = S.GRID32[S.GRID32.abs() <= 8.0].double()
    for act, f in ((L.ACT_GELU, F.gelu), (L.ACT_SIGMOID, torch.sigmoid), (L.ACT_TANH, torch.tanh), (L.ACT_ELU1, lambda t: F.elu(t) + 1.0),
                   (L.ACT_RELU, F.relu), (L.ACT_NONE, lambda t: t)):
        assert (S.act_ref(act, x) - f(x)).abs().max().item() <= 1e-15 * 8, S.ACT_NAMES[act]
    assert S.act_ref(L.ACT_GELU, torch.tensor([-40.0, 40.0, 2.0 ** 100, -2.0 ** 100])).tolist() == [-0.0, 40.0, 2.0 ** 100, -0.0]
    nan = torch.tensor([S.NAN])
    assert all(torch.isnan(S.act_ref(a, nan)).all() for a in S.ACTS)
    inf = torch.tensor([S.INF, -S.INF])
    assert S.act_ref(L.ACT_SIGMOID, inf).tolist() == [1.0, 0.0] and S.act_ref(L.ACT_TANH, inf).tolist() == [1.0, -1.0]
    assert S.act_ref(L.ACT_RELU, inf).tolist() == [S.INF, 0.0]


def test_vt_bits_match_the_library_helper():
    y = torch.cat([S.GRID32, torch.tensor(S.VT_VALUES), torch.tensor([S.NAN])])
    for fmt in (L.ATTN_P_BF16, L.ATTN_P_FP16):
        assert torch.equal(S.vt_bits(y, fmt), L.vt_image(y, fmt).view(torch.int16))
    enc = lambda v: S.vt_bits(torch.tensor([v]), 1).view(torch.float16).item()
    assert enc(65280.0) == 65280.0 and enc(65504.0) == 65504.0 and enc(65520.0) == 65504.0 and enc(1e5) == 65504.0 and enc(-1e5) == -65504.0       # bf16 first, then saturated
    assert math.isnan(enc(S.NAN))


# ------------------------------------------------------------------------------------------------ the grid
def test_grid_holds_what_it_promises():
    g = S.GRID32
    assert g.numel() == S.GRID_N == S.GRID16.numel()
    bits = g.view(torch.int32)
    assert (bits == 0).any() and (bits == -2 ** 31).any(), "+0 and -0"
    for sign in (1.0, -1.0):
        c = torch.tensor([0.125]).view(torch.int32).item()
        want = (torch.arange(c - 32, c + 33, dtype=torch.int32).view(torch.float32) * sign)
        assert all((g == v).any() for v in want), "every fp32 within 32 ulp of +-0.125"
        for lo, hi in S.EXP_SPANS:
            assert ((g * sign >= lo) & (g * sign <= hi)).sum() >= 32
        for p in S.EXP_POINTS:
            p32 = torch.tensor([p], dtype=torch.float32)
            for nb in (torch.nextafter(p32, torch.tensor([0.0])), p32, torch.nextafter(p32, torch.tensor([1e9]))):
                assert (g == nb * sign).any(), p
        assert (g == sign * 1e20).any() and (g == sign * 1e30).any()
        assert (g == sign * 2.0 ** -20).any() and ((g * sign > 109.99) & (g * sign < 110.01)).any() and (g * sign > 1e38).any()
    assert (g[-1000:].abs() <= 8.0).all() and (g[-1000:].diff() > 0).all(), "the uniform fill of [-8, 8]"
    assert not torch.isnan(g).any()


def test_grid16_is_sp_exact_and_keeps_the_branch_neighbourhood():
    import kernel_refs as R
    assert torch.equal(R.sp_round(S.GRID16).view(torch.int32), S.GRID16.view(torch.int32)), "bit for bit"
    hi, lo = R.sp_split(S.GRID16)
    assert torch.equal(hi.float() + lo.float(), S.GRID16)
    for sign in (1.0, -1.0):
        for k in range(33):
            assert (S.GRID16 == sign * (0.125 + k * 2.0 ** -18)).any() and (S.GRID16 == sign * (0.125 - k * 2.0 ** -19)).any(), k
    # the 16-bit grid is the fp32 grid rounded: nothing moved by more than 2^-16 relative, outside the rebuilt neighbourhood
    far = (S.GRID32.abs() < 0.1249) | (S.GRID32.abs() > 0.1252)
    assert ((S.GRID16 - S.GRID32).abs()[far] <= S.GRID32.abs()[far] * 2.0 ** -16).all()


def test_grid_fits_the_smallest_launch_of_each_kernel():
    for sid, (P, cin, n) in S.smallest_launches().items():
        for width in (cin, n):                                              # identity injection (over the input channels), share injection (over the couts)
            cols = S.grid_cols(width, n)
            assert P * len(cols) >= S.GRID_N, (sid, P, len(cols))
            x = S.injection(S.GRID16, P, width, n)
            seen = torch.unique(x[:, cols].contiguous().view(torch.int32))
            assert set(torch.unique(S.GRID16.view(torch.int32)).tolist()) <= set(seen.tolist()), sid
    assert min(P * len(S.grid_cols(min(cin, n), n)) for P, cin, n in S.smallest_launches().values()) == S.SMALLEST[0] * (S.SMALLEST[1] - 3)


def _ranges_seen(block: torch.Tensor) -> set:
    a = block.abs()
    return {name for name, (lo, hi) in S.RANGES.items() if ((a >= lo) & (a < hi)).any()}


@pytest.mark.parametrize("sid", list(S.SITES))
def test_every_range_in_every_cout_group_and_tile(sid):
    """the layout of each site: every 8-cout row group over the pixels -- the ragged tail's group included --, and every tile of 32
    pixels x 64 couts, holds values of every range"""
    P, cin, n = S.smallest_launches()[sid]
    for grid, width in ((S.GRID16, cin), (S.GRID32, n)):
        x = S.injection(grid, P, width, n)
        cols = S.grid_cols(width, n)
        for c0 in range(0, min(width, n), 8):
            own = [c for c in cols if c0 <= c < c0 + 8]
            assert _ranges_seen(x[:, own]) == set(S.RANGES), (sid, c0, set(S.RANGES) - _ranges_seen(x[:, own]))
        for p0 in range(0, P, 32):
            for c0 in range(0, min(width, n), 64):
                own = [c for c in cols if c0 <= c < c0 + 64]
                assert _ranges_seen(x[p0:p0 + 32, own]) == set(S.RANGES), (sid, p0, c0)


def test_special_couts_are_single_and_apart():
    for n in (54, 64, 126, 128, 190, 256, 768):
        sp = S.special_couts(n)
        assert len(set(sp.values())) == 3 and len({c // 8 for c in sp.values()}) == 3 and max(sp.values()) == n - 1
    b = S.special_bias(54, L.ACT_GELU, L.EPI_STORE)
    assert torch.isnan(b).sum() == 1 and torch.isfinite(b).sum() == 53
    b = S.special_bias(54, L.ACT_TANH, L.EPI_STORE)
    assert torch.isnan(b[53]) and b[2] == S.INF and b[11] == -S.INF


# ------------------------------------------------------------------------------------------------ emulation and wrong variants
@pytest.mark.parametrize("grid", ["grid16", "grid32"])
@pytest.mark.parametrize("kind,act", S.EPI_CASES, ids=CASE_IDS)
def test_emulation_within_half_the_bound(kind, act, grid):
    """common.h's formulas in fp32 with correctly rounded exp2 / reciprocal: inside HALF the bound everywhere, NaN and +-inf as specified"""
    v, aux, z = S.cpu_case(kind, act, S.GRID16 if grid == "grid16" else S.GRID32)
    got = S.Emulation().epilogue(kind, act, 1.0, v, aux, z)
    out = S.compare(f"emulation {S.KIND_NAMES[kind]} {S.ACT_NAMES[act]} {grid}", kind, act, 1.0, got, v, aux, z, scale_bound=0.5)
    print(out)
    assert out.ok, str(out)
    assert torch.isnan(got[:, S.special_couts(v.shape[1])["nan"]]).all()


def test_emulation_scale_quarter_is_exact():
    v, aux, z = S.cpu_case(L.EPI_STORE, L.ACT_NONE)
    out = S.compare("emulation scale", L.EPI_STORE, L.ACT_NONE, 0.25, S.Emulation().epilogue(L.EPI_STORE, L.ACT_NONE, 0.25, v), v)
    assert out.ok, str(out)


def test_emulation_worst_error_per_function():
    """the figures the log quotes: max |error| of the emulated sigmoid, tanh and GELU over the fp32 grid (the issue's 4M-point sweep found
    9.3e-8, 1.9e-7 and 1.9e-7 max(1, |x|))"""
    x = S.GRID32[torch.isfinite(S.GRID32)]
    e = S.Emulation()
    for act, bound in ((L.ACT_SIGMOID, 1.5e-7), (L.ACT_TANH, 3e-7), (L.ACT_GELU, 3e-7)):
        got = e.epilogue(L.EPI_STORE, act, 1.0, x.reshape(1, -1)).double().flatten()
        err = (got - S.act_ref(act, x)).abs() / x.double().abs().clamp_min(1.0)
        i = int(err.argmax())
        print(f"emulation {S.ACT_NAMES[act]}: max |err| / max(1, |x|) = {err[i].item():.3e} at x = {x[i].item()!r}")
        assert err[i].item() <= bound


@pytest.mark.parametrize("name", list(S.WRONG))
def test_wrong_variant_is_rejected(name):
    args, (kind, act) = S.WRONG[name]
    v, aux, z = S.cpu_case(kind, act)
    good = S.compare(name, kind, act, 1.0, S.Emulation().epilogue(kind, act, 1.0, v, aux, z), v, aux, z)
    bad = S.compare(name, kind, act, 1.0, S.Emulation(**args).epilogue(kind, act, 1.0, v, aux, z), v, aux, z)
    print(bad)
    assert good.ok and not bad.ok, f"{name} passes the sweep: {bad}"


# ------------------------------------------------------------------------------------------------ convex upsampling reference
@pytest.mark.parametrize("case", S.CONVEX_LOGITS)
def test_convex_reference_is_the_oracle_formula(case):
    """the tap-by-tap float64 reference against the oracle's closed forms evaluated in float64 (2-D, and 3-D without halo frames); with halo
    frames: against the oracle on the extended volume whose mask is zero outside the own frames"""
    from oracle import ppm_oracle as O
    from ppmstereo_amd.weights import hash_normal
    T, H, W = 2, 5, 9
    P = T * H * W
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    fl, m = hash_normal((T, H, W, 2), 61), S.convex_logits(case, P, 9, 62).reshape(T, H, W, 144)
    assert (S.convex_upsample(fl, m) - O.convex_upsample(nchw(fl), nchw(m))).abs().max().item() <= 1e-13
    m = S.convex_logits(case, P, 27, 63).reshape(T, H, W, 432)
    assert (S.convex_upsample(fl, m) - O.convex_upsample_3d(nchw(fl), nchw(m), 4, T)).abs().max().item() <= 1e-13
    fe = hash_normal((T + 2, H, W, 2), 64)
    me = torch.zeros(T + 2, H, W, 432)
    me[1:T + 1] = m
    assert (S.convex_upsample(fe, m, 1) - O.convex_upsample_3d(nchw(fe), nchw(me), 4, T + 2)[1:T + 1]).abs().max().item() <= 1e-13
    lg = S.convex_logits(case, P, 27, 65).reshape(P, 27, 16)
    if case == "all_equal":
        assert (lg == lg[:, :1]).all()
    if case == "one_tap_+80":
        assert ((lg.max(1).values - lg.median(1).values) > 70).all()
    if case == "one_tap_-1e4":
        assert ((lg == -1e4).sum(1) == 1).all()


def test_dwconv_sweep_inputs_hold_the_grid():
    for k in S.DWG_SWEEP:
        x = S.dwg_sweep_input(k)
        assert set(torch.unique(S.GRID16.view(torch.int32)).tolist()) <= set(torch.unique(x.contiguous().view(torch.int32)).tolist())
