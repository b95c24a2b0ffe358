"""CPU: the float64 references of tests/kernel_refs.py against the corresponding torch ops (to float64 rounding), and -- on the exact
inputs and with the tolerance rule of every GPU case of test_gpu_encoder_ops.py / test_gpu_glue_ops.py / test_gpu_update_ops.py /
test_gpu_memory_ops.py / test_gpu_flow_ops.py -- shown sensitive to the mistakes they exist to catch: every named wrong variant exceeds the
tolerance on at least one case of its kernel, while the reference itself and the plain fp32 torch form stay inside it.  That is a condition
on the cases, not a measurement: where a variant slips through, the inputs change, not the tolerance.  The last part covers the correlation
pyramid build, the convex upsamplings, the tap gather-sum, the bilinear resize and the inputs of the transposes."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
from ppmstereo_amd.weights import hash_normal

F64 = torch.float64


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a.double() - b.double()).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), err


# ------------------------------------------------------------------------------------------------ references vs torch
def test_slices_rederived():
    """the shape arithmetic of the instnorm / GRN cases: (S, chunk) of in_slices_host"""
    assert R.in_slices(1, 4225, 64) == (66, 65) and 65 * 65 == 4225            # A: slice 65 is empty; 66 = 8 * 8 + 2
    assert R.in_slices(2, 35, 96) == (1, 35)                                    # B
    assert R.in_slices(3, 700, 40) == (10, 70)                                  # C
    assert R.in_slices(1, 130, 30) == (2, 65)                                   # D
    assert R.in_slices(1, 130, 3072) == (2, 65)                                 # GRN, C > 256


def test_instnorm_vs_torch():
    x = hash_normal((2, 45, 24), 1).double() * 3 + 1
    res = hash_normal((2, 45, 24), 2).double()
    mean, rstd, y = R.instnorm(x, 1e-5)
    close(y, F.instance_norm(x.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1))
    close(mean, x.mean(1))
    close(rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5))
    close(R.instnorm(x, 1e-5, res, True)[2], F.relu(F.instance_norm(x.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1) + res))


def test_layernorm_vs_torch():
    x, w, b = hash_normal((37, 40), 3).double() * 2 + 5, hash_normal((40,), 4).double(), hash_normal((40,), 5).double()
    close(R.layernorm(x, w, b, 1e-6), F.layer_norm(x, (40,), w, b, 1e-6))


def test_grn_vs_oracle_expression():
    """the expression of oracle.ppm_oracle.convnext_block, on its (N, H, W, C) layout"""
    h = hash_normal((2, 5, 7, 24), 6).double()
    gamma, beta = hash_normal((24,), 7).double(), hash_normal((24,), 8).double()
    gx = torch.norm(h, p=2, dim=(1, 2), keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    want = gamma * (h * nx) + beta + h
    close(R.grn(h.reshape(2, 35, 24), gamma, beta), want.reshape(2, 35, 24))


def test_dwconv_vs_torch():
    x, w, b = hash_normal((2, 5, 9, 16), 9).double(), hash_normal((16, 49), 10).double(), hash_normal((16,), 11).double()
    want = F.conv2d(x.permute(0, 3, 1, 2), w.reshape(16, 1, 7, 7), b, padding=3, groups=16).permute(0, 2, 3, 1)
    close(R.dwconv(x, w, b), want)


@pytest.mark.parametrize("k", [2, 4])
def test_s2d_vs_pixel_unshuffle(k):
    x = hash_normal((2, 8, 12, 5), 12).double()
    pu = F.pixel_unshuffle(x.permute(0, 3, 1, 2), k)                            # channel c k k + (k dy + dx)
    want = pu.reshape(2, 5, k * k, 8 // k, 12 // k).permute(0, 3, 4, 2, 1).reshape(2, 8 // k, 12 // k, k * k * 5)      # -> phase C + c
    assert torch.equal(R.s2d(x, k), want)


def test_upsample_vs_interpolate():
    x = hash_normal((2, 3, 5, 4), 13).double()
    want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.upsample2(x), want)


def test_flow_patch_vs_unfold():
    flow = hash_normal((2, 5, 9, 2), 14).double()
    u = F.unfold(flow.permute(0, 3, 1, 2), 7, padding=3)                        # (BT, c 49 + tap, HW)
    want = u.reshape(2, 2, 49, 45).permute(0, 3, 2, 1).reshape(2, 5, 9, 98)
    got = R.flow_patch(flow)
    assert torch.equal(got[..., :98], want) and (got[..., 98:] == 0).all() and got.shape[-1] == 128


@pytest.mark.parametrize("case", R.RESIZE_CASES)
def test_resize_vs_interpolate(case):
    N, H, W, OH, OW = case
    dst, src = (t.double() for t in R.resize_inputs(case))
    want = F.interpolate(src.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    close(R.resize_blend(dst, src, OH, OW, 0.0, 1.0), want)
    close(R.resize_blend(dst, src, OH, OW, 0.5, 0.5), 0.5 * dst + 0.5 * want)
    nan = torch.full_like(dst, float("nan"))
    assert torch.isfinite(R.resize_blend(nan, src, OH, OW, 0.0, 1.0)).all()


@pytest.mark.parametrize("case", R.AVGPOOL_CASES)
def test_avgpool_vs_torch(case):
    x = R.avgpool_input(case).double()
    close(R.avgpool(x, case[0]), F.avg_pool2d(x[None], case[0], stride=case[0])[0])


def test_small_refs_vs_torch():
    x, y = hash_normal((12,), 15).double(), hash_normal((4,), 16).double()
    close(R.axpby(x, y, 0.5, 2.0, 4), 0.5 * x + 2.0 * y.repeat(3))
    f, c = hash_normal((2, 256, 35), 17).double(), hash_normal((2, 256, 35), 18).double()
    net, inp = R.ctx_mix(f, c)
    close(net, torch.tanh((f[:, :128] + c[:, :128]) / 2))
    close(inp, F.relu((f[:, 128:] + c[:, 128:]) / 2))
    xs, w, b = R.unc_inputs((2, 700))
    unc, part = R.unc_tail(xs, w, b)
    close(unc, torch.sigmoid(F.linear(xs.double(), w.double()[None]).squeeze(-1) + b))
    assert part.shape == (2, 3)
    close(part[:, 2], unc[:, 512:].sum(1))
    close(part.sum(1), unc.sum(1))


def test_sp_split_bound():
    """the split planes: |hi + lo - x| <= 2^-16 |x|, and a pair read back is reproduced exactly"""
    x = hash_normal((1 << 14,), 19) * 5
    hi, lo = R.sp_split(x)
    assert R.split_check(R.Check(), "x", hi, lo, x).ok
    assert torch.equal(R.sp_round(R.sp_round(x)), R.sp_round(x))


# ------------------------------------------------------------------------------------------------ every wrong variant is caught
def _instnorm_runs(fn):
    """Check of fn over every (case, data, residual, relu) the GPU test runs; None where the variant does not apply"""
    out = []
    for case in R.INSTNORM_CASES:
        for data in ("unit", "offset"):
            x, res = R.instnorm_inputs(case, data)
            for with_res in (False, True):
                for relu in (False, True):
                    got = fn(x, R.IN_EPS, res[:, :, :x.shape[2]] if with_res else None, relu)
                    if got is not None:
                        out.append(R.instnorm_check(case, data, with_res, relu, *got))
    return out


def test_instnorm_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _instnorm_runs(R.instnorm))
    runs = _instnorm_runs(R.instnorm_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.INSTNORM_WRONG))
def test_instnorm_wrong_variant_is_caught(name):
    runs = _instnorm_runs(R.INSTNORM_WRONG[name])
    assert runs and any(not c.ok for c in runs), name


def test_instnorm_needs_both_kinds_of_data():
    """on unit data the applied result lets eps = 1e-6 through (only the rstd column of the stats shows it) and catches the unbiased variance;
    on offset data the applied result catches eps = 1e-6 and the one-pass variance"""
    y_ok = lambda ck: all(e <= t for n, e, t in ck.items if n == "y")
    unit = lambda fn: [R.instnorm_check("A", "unit", False, False, *fn(R.instnorm_inputs("A", "unit")[0], R.IN_EPS))]
    offs = lambda fn: [R.instnorm_check("A", "offset", False, False, *fn(R.instnorm_inputs("A", "offset")[0], R.IN_EPS))]
    assert not unit(R.INSTNORM_WRONG["unbiased"])[0].ok
    eps_unit, eps_offs = unit(R.INSTNORM_WRONG["eps_1e-6"])[0], offs(R.INSTNORM_WRONG["eps_1e-6"])[0]
    assert y_ok(eps_unit) and not eps_unit.ok and not y_ok(eps_offs)
    assert not y_ok(unit(R.INSTNORM_WRONG["unbiased"])[0]) and not y_ok(offs(R.INSTNORM_WRONG["one_pass_fp32"])[0])
    assert not offs(R.INSTNORM_WRONG["eps_1e-6"])[0].ok and not offs(R.INSTNORM_WRONG["one_pass_fp32"])[0].ok


@pytest.mark.parametrize("name", list(R.GRN_WRONG))
def test_grn_wrong_variant_is_caught(name):
    runs = [R.grn_check(case, R.GRN_WRONG[name](*R.grn_inputs(case))) for case in R.GRN_CASES]
    assert any(not c.ok for c in runs), name


def test_grn_cases_pass_the_reference_and_fp32():
    for case in R.GRN_CASES:
        assert R.grn_check(case, R.grn(*R.grn_inputs(case))).ok
        ck = R.grn_check(case, R.grn_f32(*R.grn_inputs(case)))
        assert ck.ok, str(ck)


def test_grn_eps_needs_the_tiny_case():
    assert not R.grn_check("tiny", R.GRN_WRONG["eps_1e-5"](*R.grn_inputs("tiny"))).ok
    assert R.grn_check("small", R.GRN_WRONG["eps_1e-5"](*R.grn_inputs("small"))).ok      # invisible at unit magnitude


@pytest.mark.parametrize("name", list(R.LN_WRONG))
def test_layernorm_wrong_variant_is_caught(name):
    for C in R.LN_CASES:                                                                  # (here: on every case)
        ck = R.layernorm_check(C, R.LN_WRONG[name](*R.layernorm_inputs(C), R.LN_EPS))
        assert not ck.ok, (name, C)


def test_layernorm_cases_pass_the_reference_and_fp32():
    for C in R.LN_CASES:
        assert R.layernorm_check(C, R.layernorm(*R.layernorm_inputs(C), R.LN_EPS)).ok
        ck = R.layernorm_check(C, R.layernorm_f32(*R.layernorm_inputs(C), R.LN_EPS))
        assert ck.ok, str(ck)


@pytest.mark.parametrize("name", list(R.DW_WRONG))
def test_dwconv_wrong_variant_is_caught(name):
    runs = [R.dwconv_check(case, R.DW_WRONG[name](*R.dwconv_inputs(case))) for case in R.DW_CASES]
    assert all(not c.ok for c in runs), name


def test_dwconv_cases_pass_fp32():
    for case in R.DW_CASES:
        ck = R.dwconv_check(case, R.dwconv_f32(*R.dwconv_inputs(case)))
        assert ck.ok, str(ck)


def test_layout_wrong_variants_are_caught():
    for case in R.S2D_CASES:
        N, H, W, C = case
        x = R.s2d_input(case).reshape(N, H, W, C)
        assert not R.Check().exact("s2d", R.S2D_WRONG["dy_dx_swapped"](x, 2), R.s2d(x, 2)).ok
    for k, shape, c in R.IMG_S2D_CASES:
        x = R.img_input(shape).permute(0, 2, 3, 1)
        assert not R.Check().exact("img_s2d", R.S2D_WRONG["dy_dx_swapped"](x, k), R.s2d(x, k)).ok
    x = R.upsample_input().reshape(*R.UP_CASE, 32)[..., 8:24]
    assert not R.Check().exact("up", R.UP_WRONG["(y+1)>>1"](x), R.upsample2(x)).ok
    for case in R.PATCH_CASES:
        flow = R.flow_input(case)
        assert not R.Check().exact("patch", R.PATCH_WRONG["tap=kx*7+ky"](flow), R.flow_patch(flow)).ok


def test_resize_wrong_variant_is_caught():
    caught = 0
    for case in R.RESIZE_CASES:
        for a, b in R.RESIZE_AB:
            dst, src = R.resize_inputs(case)
            ref = R.resize_blend(dst, src, case[3], case[4], a, b)
            caught += not R.Check().add("y", R.RESIZE_WRONG["align_corners=False"](dst, src, case[3], case[4], a, b), ref, R.tol_sp(ref)).ok
    assert caught >= 4                                                        # every case but the identity, both blends


def test_avgpool_wrong_variant_is_caught():
    runs = []
    for case in R.AVGPOOL_CASES:
        x = R.avgpool_input(case)
        ref = R.avgpool(x, case[0])
        runs.append(R.Check().add("y", R.AVGPOOL_WRONG["clipped_divisor"](x, case[0]), ref, R.tol_reduce(ref, R.avgpool_f32(x, case[0]), False)))
    assert any(not c.ok for c in runs)


# ================================================================================================ kernels of the update iteration
# ------------------------------------------------------------------------------------------------ references vs torch / the oracle
@pytest.mark.parametrize("case", list(R.LOOKUP_CASES))
def test_corr_lookup_vs_grid_sample_and_oracle(case):
    """the float64 lookup against F.grid_sample (align_corners=True, zero padding) on the normalised positions, and against the oracle's
    corr_lookup fed float64 (which returns fp32: compared at fp32 rounding)"""
    from oracle import ppm_oracle as O
    B, H, W = R.LOOKUP_CASES[case]
    levels, flow = R.lookup_inputs(case)
    got = R.corr_lookup(levels, flow[:, 0], W)
    P = B * H * W
    xs = (torch.arange(P) % W).double() + flow[:, 0].double()
    for l, L in enumerate(levels):
        Wl = L.shape[1]
        p = (torch.arange(9, dtype=F64) - 4)[None] + xs[:, None] / 2 ** l
        grid = torch.stack([2 * p / (Wl - 1) - 1, torch.zeros_like(p)], -1).reshape(P, 1, 9, 2)
        want = F.grid_sample(L.double().reshape(P, 1, 1, Wl), grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(P, 9)
        close(got[:, 9 * l:9 * l + 9], want, 1e-9)
    pyr = [L.double() for L in levels]
    want = O.corr_lookup(pyr, flow.double().reshape(B, H, W, 2).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(P, 36)
    close(got, want, 1e-6)


def test_lookup_flow_recipe():
    """what the flow of the lookup cases is built to contain"""
    for case, (B, H, W) in R.LOOKUP_CASES.items():
        levels, flow = R.lookup_inputs(case)
        P = B * H * W
        assert P >= 11 and torch.isfinite(flow).all()
        ref = R.lookup_refs(case)[0]
        for l in range(4):
            assert ref[1 + 2 * l, 9 * l] == levels[l][1 + 2 * l, -1].double() and (ref[1 + 2 * l, 9 * l + 1:9 * l + 9] == 0).all()      # tap 0 on column Wl - 1
            assert ref[2 + 2 * l, 9 * l + 8] == levels[l][2 + 2 * l, 0].double() and (ref[2 + 2 * l, 9 * l:9 * l + 8] == 0).all()        # tap 8 on column 0
        assert (ref[9] == 0).all() and (ref[10] == 0).all() and flow[9, 0] == 1e9 and flow[10, 0] == -1e9
        x = torch.arange(P) % W
        plain = torch.ones(P, dtype=torch.bool)
        plain[1:11] = False
        assert (flow[(x % 5 == 0) & (x % 7 != 0) & plain, 0] % 1 == 0).all()
    assert [R.LOOKUP_CASES["P54"][2] >> l for l in range(4)] == [18, 9, 4, 2] and (1 * 3 * 18) % 4 == 2


def _pcblock_weights(c, hid, cout):
    mk = lambda shape, seed, fan: hash_normal(shape, seed).double() / fan ** 0.5
    W, p = {}, "p."
    for name, shape, fan, seed in (("ffn1.0", (hid, c, 1, 1), c, 30), ("ffn1.2", (c, hid, 1, 1), hid, 32), ("conv_list.0", (c, 1, 1, 1), 4, 34),
                                   ("conv_list.1", (c, 1, 7, 7), 49, 36), ("pw", (c, c, 1, 1), c, 38), ("ffn2.0", (hid, c, 1, 1), c, 40),
                                   ("ffn2.2", (cout, hid, 1, 1), hid, 42)):
        W[p + name + ".weight"], W[p + name + ".bias"] = mk(shape, seed, fan), 0.1 * hash_normal((shape[0],), seed + 1).double()
    return W


def test_pwchain_and_dwconv_gelu_vs_oracle_pcblock():
    """chain A, the depthwise 7 x 7 + GELU and chain B in sequence are gelu(PCBlock4_Deep_nopool_res.forward) of the oracle"""
    from oracle import ppm_oracle as O
    c, hid, cout, BT, H, Wd = 12, 20, 24, 2, 5, 9
    W = _pcblock_weights(c, hid, cout)
    x = hash_normal((BT, c, H, Wd), 29).double()
    want = F.gelu(O.pcblock(W, "p", x)).permute(0, 2, 3, 1)
    g = lambda n: (W[f"p.{n}.weight"].reshape(W[f"p.{n}.weight"].shape[0], -1), W[f"p.{n}.bias"])
    rows = x.permute(0, 2, 3, 1).reshape(-1, c)
    a = R.pwchain(rows, [(*g("ffn1.0"), False, None), (*g("ffn1.2"), True, (W["p.conv_list.0.weight"].reshape(c), W["p.conv_list.0.bias"]))])
    d = R.dwconv_gelu(a.reshape(BT, H, Wd, c), *g("conv_list.1"), 7)
    b = R.pwchain(d.reshape(-1, c), [(*g("pw"), True, None), (*g("ffn2.0"), False, None), (*g("ffn2.2"), False, None)])
    close(b.reshape(BT, H, Wd, cout), want)
    close(R.dwconv_gelu(x.permute(0, 2, 3, 1), W["p.conv_list.0.weight"].reshape(c, 1), W["p.conv_list.0.bias"], 1),
          F.gelu(x + O._c2(W, "p.conv_list.0", x, 0, groups=c)).permute(0, 2, 3, 1))


@pytest.mark.parametrize("C", [256, 384])
def test_time_attn_vs_oracle(C):
    """the oracle's TimeAttnBlock with identity proj / fc layers is x + the attention core"""
    from oracle import ppm_oracle as O
    T, h, w = 3, 2, 5
    x = hash_normal((T, C, h, w), 50 + C).double()
    W = {"time_attn.temporal_norm1.weight": 1 + 0.1 * hash_normal((C,), 51).double(), "time_attn.temporal_norm1.bias": 0.1 * hash_normal((C,), 52).double(),
         "time_attn.temporal_attn.proj.weight": torch.eye(C, dtype=F64), "time_attn.temporal_attn.proj.bias": torch.zeros(C, dtype=F64),
         "time_attn.temporal_fc.weight": torch.eye(C, dtype=F64), "time_attn.temporal_fc.bias": torch.zeros(C, dtype=F64)}
    want = (O.time_attn(W, x, T) - x).permute(0, 2, 3, 1).reshape(T, h * w, C)
    got = R.time_attn(x.permute(0, 2, 3, 1).reshape(T, h * w, C), W["time_attn.temporal_norm1.weight"], W["time_attn.temporal_norm1.bias"])
    close(got, want, 1e-11)


def test_layernorm16_and_linear_attention_vs_torch():
    from oracle import ppm_oracle as O
    x, w, b, r = (hash_normal(s, 60 + i).double() for i, s in enumerate([(7, 256), (256,), (256,), (7, 256)]))
    close(R.layernorm16(x, w, b), O.layer_norm(x, w, b))
    close(R.layernorm16(x, w, b, r), r + F.layer_norm(x, (256,), w, b, 1e-5))
    Q, K, V = (t.double() for t in R.linattn_inputs(32, (2, 77), "unit"))
    S = 77                                                                     # LinearAttention.forward as the oracle's loftr_layer states it
    KV = torch.einsum("nshd,nshv->nhdv", K, V)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(1)) + 1e-6)
    close(R.linear_attention(Q, K, V), torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * S)


def test_update_case_arithmetic():
    """the shape arithmetic the case tables rely on"""
    assert [(n + 3) // 4 for _, n in R.LA_CASES] == [1, 20, 161] and 161 == R.LA_PASS + 1 and 77 % 32 == 13
    assert R._la_keep(3, "last_split") is None and R._la_keep(77, "first_pass") is None and R._la_keep(644, "first_pass").sum() == 640
    assert R.LN16_PIXELS % 4 == 3 and 16384 in R.PW_PIXELS and 16385 % 128 == 1
    BT, H, W, c, ld, k = R.DWG_CASES["edges"]
    assert H <= k // 2 and W <= k and W % 2 == 1 and BT > 1


# ------------------------------------------------------------------------------------------------ every wrong variant is caught
def _lookup_runs(fn):
    out = []
    for case, (B, H, W) in R.LOOKUP_CASES.items():
        levels, flow = R.lookup_inputs(case)
        got = fn(levels, flow, B, H, W)
        out += [R.lookup_check(case, got, True), R.lookup_check(case, got, False)]      # the SP outputs' tolerance and the fp32 output's
    return out


def test_lookup_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _lookup_runs(lambda lv, fl, B, H, W: R.corr_lookup(lv, fl[:, 0], W)))
    runs = _lookup_runs(R.corr_lookup_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.LOOKUP_WRONG))
def test_lookup_wrong_variant_is_caught(name):
    runs = _lookup_runs(lambda lv, fl, B, H, W: R.LOOKUP_WRONG[name](lv, fl[:, 0], W))
    assert all(not c.ok for c in runs), name                                            # (here: on every case)


def test_dwg_cases_pass_the_reference_and_fp32():
    for case in R.DWG_CASES:
        ref, f32 = R.dwg_refs(case)
        assert R.dwg_check(case, ref).ok
        ck = R.dwg_check(case, f32)
        assert ck.ok, str(ck)


@pytest.mark.parametrize("name", list(R.DWG_WRONG))
def test_dwg_wrong_variant_is_caught(name):
    runs = [R.dwg_check(case, R.dwconv_gelu(*R.dwg_inputs(case), R.DWG_CASES[case][5], **R.DWG_WRONG[name])) for case in R.DWG_CASES]
    assert any(not c.ok for c in runs), name
    if name in ("zero_padding_in_y_only", "no_frame_boundary", "replicate_padding"):
        assert not runs[list(R.DWG_CASES).index("edges")].ok                           # what the "edges" case is for


def test_pwchain_cases_pass_the_reference_and_fp32():
    for chain, (cin, _, _) in R.PW_CHAINS.items():
        for P in R.PW_PIXELS:
            assert R.pwchain_check(chain, P, R.pwchain_ref(chain)[:P]).ok
        ck = R.pwchain_check(chain, 16385, R.pwchain_f32(R.pwchain_input()[:, :cin], R.pwchain_layers(chain)))
        assert ck.ok, str(ck)


@pytest.mark.parametrize("name", list(R.PW_WRONG))
def test_pwchain_wrong_variant_is_caught(name):
    runs = []
    for chain, (cin, _, _) in R.PW_CHAINS.items():
        got = R.pwchain(R.pwchain_input()[:318, :cin], R.pwchain_layers(chain), **R.PW_WRONG[name])
        runs.append(R.pwchain_check(chain, 318, got))
    assert any(not c.ok for c in runs), name


def _ta_runs(fn, data_kinds=R.A16_DATA):
    return [R.time_attn_check(C, case, data, fn(*R.time_attn_inputs(C, case, data))) for C in (256, 384) for case in R.TA_CASES for data in data_kinds]


def test_time_attn_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _ta_runs(R.time_attn))
    runs = _ta_runs(R.time_attn_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.TA_WRONG))
def test_time_attn_wrong_variant_is_caught(name):
    runs = _ta_runs(R.TA_WRONG[name])
    assert any(not c.ok for c in runs), name
    for C in (256, 384):                                                                # both instantiations see every mistake
        assert any(not c.ok for c in runs if f"C={C}" in c.label), (name, C)


def test_time_attn_eps_needs_the_flat_data():
    assert all(not c.ok for c in _ta_runs(R.TA_WRONG["eps_1e-6"], ("flat",)))
    assert all(c.ok for c in _ta_runs(R.TA_WRONG["eps_1e-6"], ("unit",)))               # invisible at unit variance


def _ln16_runs(fn, data_kinds=R.A16_DATA):
    out = []
    for C in (256, 384):
        for data in data_kinds:
            x, w, b, res = R.layernorm16_inputs(C, data)
            for with_res in (False, True):
                got = fn(x, w, b, res if with_res else None)
                if got is not None:
                    out.append(R.layernorm16_check(C, data, with_res, got))
    return out


def test_layernorm16_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _ln16_runs(R.layernorm16))
    runs = _ln16_runs(R.layernorm16_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.LN16_WRONG))
def test_layernorm16_wrong_variant_is_caught(name):
    runs = _ln16_runs(R.LN16_WRONG[name])
    assert runs and any(not c.ok for c in runs), name
    for C in (256, 384):
        assert any(not c.ok for c in runs if f"C={C}" in c.label), (name, C)
    if name == "eps_1e-6":
        assert all(not c.ok for c in _ln16_runs(R.LN16_WRONG[name], ("flat",)))


def _la_runs(fn, data_kinds=R.LA_DATA):
    out = []
    for dh in (32, 48):
        for case in R.LA_CASES:
            for data in data_kinds:
                got = fn(*R.linattn_inputs(dh, case, data))
                if got is not None:
                    out.append(R.linattn_check(dh, case, data, got))
    return out


def test_linattn_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _la_runs(R.linear_attention))
    runs = _la_runs(R.linear_attention_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.LA_WRONG))
def test_linattn_wrong_variant_is_caught(name):
    runs = _la_runs(R.LA_WRONG[name])
    assert runs and any(not c.ok for c in runs), name
    for dh in (32, 48):
        assert any(not c.ok for c in runs if f"dh={dh}" in c.label), (name, dh)


def test_linattn_eps_needs_the_tiny_data():
    runs = _la_runs(R.LA_WRONG["no_divisor_eps"], ("tiny",))
    assert all(not c.ok for c in runs if "644" not in c.label)                          # n = 3 and 77; at n = 644 Q . sum K is 0.03, the eps 3e-5 of it
    assert all(c.ok for c in _la_runs(R.LA_WRONG["no_divisor_eps"], ("unit",)))         # invisible at unit-scale K


# ================================================================================================ memory read-out
# ------------------------------------------------------------------------------------------------ references vs the oracle
def test_mem_scale():
    from oracle import ppm_oracle as O
    from ppmstereo_amd.engine import softmax_scale
    assert R.MEM_SCALE == O.softmax_scale(128) == softmax_scale(128)


@pytest.mark.parametrize("case", [(2, 5, 7), (9, 13, 22), (2, 23, 40)])
def test_similarity_vs_oracle(case):
    """the float64 windows, channel mean and cosine against oracle.qk_similarity fed float64 (F.adaptive_max_pool2d, F.cosine_similarity)"""
    from oracle import ppm_oracle as O
    q, k = R.sim_inputs(case, "unit")
    qbar, kbar, sim = R.qk_similarity(q, k)
    nchw = lambda x: x.double().permute(0, 3, 1, 2)
    close(sim, O.qk_similarity(nchw(q), nchw(k)))
    H, W = case[1:]
    close(qbar, F.adaptive_max_pool2d(nchw(q), (H // 4, W // 4)).mean(1).reshape(q.shape[0], -1))
    q, k = R.sim_inputs(case, "edge")                                      # a zero frame: cos = 0 by the clamp of each norm, as torch gives it
    sim = R.qk_similarity(q, k)[2]
    close(sim, O.qk_similarity(nchw(q), nchw(k)))
    assert torch.isfinite(sim).all() and (sim[0] == 0).all() and (sim[:, 0] == 0).all() and sim[1, 1].abs() > 0.1


@pytest.mark.parametrize("T", [6, 9, 40])
def test_pick_vs_oracle(T):
    """every iteration of the case against oracle.qam_select and the s_hat of oracle.play_inputs, fed float64 (no ties in these inputs)"""
    from oracle import ppm_oracle as O
    sim, parts, HW = R.pick_inputs(T)
    for (strive, ref, _), part in zip(R.pick_refs(T), parts):
        score, mask, new = O.qam_select(sim.double(), strive, part.double().sum(1) / HW)
        close(ref[0], score)
        assert torch.equal(ref[3], new)
        for i in range(T):
            J = torch.nonzero(mask[i]).flatten()
            assert ref[1][i].tolist() == J.tolist()
            z = torch.zeros(T, 4, 1, 1, dtype=F64)
            s_hat = O.play_inputs(z, z, torch.zeros(T, 4, dtype=F64), z, score, mask, i)[4]
            close(ref[2][i], s_hat)


def test_operands_vs_oracle_play_inputs():
    """prep_q / prep_k are bit for bit the bf16 rounding of play_inputs' fp32 Q and K'"""
    from oracle import ppm_oracle as O
    T, h, w = 6, 2, 5
    q, key, pe = hash_normal((T, 128, h, w), 70), hash_normal((T, 128, h, w), 71), torch.sin(hash_normal((T, 128), 72))
    score = 1.0 + 0.3 * torch.tanh(hash_normal((T, T), 73))
    mask = torch.zeros(T, T, dtype=torch.bool).scatter_(1, torch.argsort(score, 1, descending=True)[:, :5], True)
    cl = lambda x: x.permute(0, 2, 3, 1).reshape(T, h * w, 128)
    sel, shat = torch.zeros(T, 5, dtype=torch.int32), torch.zeros(T, 5)
    ops = [O.play_inputs(q, key, pe, key, score, mask, i) for i in range(T)]
    for i, (_, _, _, J, s_hat) in enumerate(ops):
        sel[i], shat[i] = J.int(), s_hat
    qb, kb = R.prep_q(cl(q), pe), R.prep_k(cl(key), pe, sel, shat, 5)
    for i, (Q, K, _, _, _) in enumerate(ops):
        assert torch.equal(qb[i], Q.to(torch.bfloat16)) and torch.equal(kb[i].reshape(-1, 128), K.to(torch.bfloat16))


def test_mem_attn_vs_oracle_flash_attn_math():
    from oracle import ppm_oracle as O
    name = ("table", 32, 36, 3)
    (q, k, v, sel, ksel, mf), scale = R.attn_named_inputs(*name)
    x, _ = R.attn_ref(*name)
    f32 = R.mem_attn_f32(q, k, v, sel, ksel, scale)
    for i in range(q.shape[0]):
        V = torch.cat([v[int(sel[i, s])].t() for s in range(ksel)], 0)
        want = O.flash_attn_math(q[i], k[i].reshape(-1, 128), V, scale)
        assert torch.equal(f32[i].float(), want)
        assert ((want.double() - x[i]).abs() <= 2.0 ** -8 * x[i].abs() + 1e-6).all()       # the oracle's result is the bf16 rounding of x


def test_memory_case_arithmetic():
    """what the case tables are built to contain"""
    assert all(R.pick_hw(nb) > 256 * (nb - 1) for nb in R.PICK_CASES.values()) and R.pick_hw(3) == 700
    assert R.PICK_CASES[9] == 65 and R.PICK_CASES[40] == 130 and set(R.PICK_CASES.values()) == {1, 3, 64, 65, 80, 130}
    assert [n // 64 for n in R.ATTN64_N] == [1, 2, 3, 5] and 60 % 8 and not 72 % 8 and 72 % 64
    # n = 320, ksel = 5, two frames per workgroup: 2 query blocks x 3 clips x 3 splits = 18 workgroups, 12 of them with two frames
    gx, nsp, nfull = (320 + 255) // 256, (5 + 1) // 2, 5 // 2
    assert gx * R.ATTN64_T * nsp == 18 and gx * R.ATTN64_T * nfull == 12 and 18 & 7 and 12 & 7
    for kernel in (32, 64):
        T, Tg, n, ksel, _ = R.ATTN_SHARDED[kernel]
        sel = R.attn_named_inputs("sharded", kernel)[0][3]
        assert Tg > T and int(sel.max()) == Tg - 1 and (n % 64 == 0) == (kernel == 64)
    for name in (("table", 32, 4, 5), ("table", 64, 320, 3), ("fixup",)):
        sel, ksel = R.attn_named_inputs(*name)[0][3:5]
        for row in sel[:, :ksel].tolist():
            assert row == sorted(set(row)) and row != list(range(ksel))
    # the 64-query kernel flags a tile whose scores rise 2^16 (fp16 P~) above the first keys' maximum: no score of its table's inputs can
    for name in [("table", 64, n, ksel) for n in R.ATTN64_N for ksel in R.ATTN64_KSEL] + [("sharded", 64)]:
        (q, k, *_), scale = R.attn_named_inputs(*name)
        s = torch.einsum("tqc,tskc->tqsk", q.double(), k.double()) * (scale / math.log(2.0))
        assert (s.amax((2, 3)) - s.amin((2, 3))).max() < 16.0, name
    q, k = R.fixup_inputs()[:2]
    s = torch.einsum("qc,skc->qsk", q[0].double(), k[0].double())
    assert s[:256].abs().max() < 8 and (s[256:, R.FIXUP_SLOT].max(1).values > 250).all() and s[256:, [0, 1, 3, 4]].abs().max() < 8
    assert torch.einsum("qc,skc->qsk", q[1].double(), k[1].double()).abs().max() < 8


# ------------------------------------------------------------------------------------------------ similarity: cases and wrong variants
def _sim_runs(fn, data_kinds=R.SIM_DATA):
    out = []
    for case in R.SIM_CASES:
        for data in data_kinds:
            for frames in (case[0], case[0] + R.SIM_EXTRA):
                q, k = R.sim_inputs(case, data)
                qbar, kbar, sim = fn(q[:frames], k[:frames])
                out.append(R.sim_check(case, data, frames, sim, torch.stack([qbar, kbar])))
    return out


def test_similarity_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _sim_runs(R.qk_similarity))
    runs = _sim_runs(R.qk_similarity_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.SIM_WRONG))
def test_similarity_wrong_variant_is_caught(name):
    runs = _sim_runs(lambda q, k: R.qk_similarity(q, k, **R.SIM_WRONG[name]))
    assert any(not c.ok for c in runs), name
    if name == "eps_on_the_product":                                       # only the tiny frame shows it
        assert all(c.ok for c in _sim_runs(lambda q, k: R.qk_similarity(q, k, **R.SIM_WRONG[name]), ("unit",)))
    if name == "fixed_4x4_windows":                                        # the maps with a remainder
        assert all(c.ok == (case[1] % 4 == 0 and case[2] % 4 == 0) for c, case in zip(runs[::4], R.SIM_CASES))


# ------------------------------------------------------------------------------------------------ pick: cases, near ties, wrong variants
def _pick_runs(results_of):
    """results_of(T) -> per iteration (score, sel, shat, new counter)"""
    out = []
    for T in R.PICK_CASES:
        ck = R.Check(f"qam pick T={T}")
        for it, res in enumerate(results_of(T)):
            R.pick_check(T, it, *res, ck=ck)
        out.append(ck)
    return out


def test_pick_cases_pass_the_reference_and_fp32():
    assert all(c.ok for c in _pick_runs(lambda T: [ref for _, ref, _ in R.pick_refs(T)]))
    runs = _pick_runs(lambda T: [f32 for _, _, f32 in R.pick_refs(T)])
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]
    for T in R.PICK_CASES:                                                 # the counter really evolved
        assert R.pick_refs(T)[-1][1][3].sum().item() == T * T + R.PICK_ITERS * T * min(5, T)


@pytest.mark.parametrize("T", list(R.PICK_CASES))
def test_pick_cases_have_no_near_tie(T):
    """every case, iteration and row with T > 5: the float64 gap between the 5th and the 6th score is at least 256 x the largest fp32-torch
    score error of the case, so an ulp of expf cannot change a pick.  A seed that fails is replaced; no row is left out."""
    gap, err = R.pick_near_tie(T)
    print(f"T={T}: gap {gap:.3e}, fp32 score error {err:.3e}")
    assert err < 2.5e-7
    assert T <= R.TOP_K or gap >= 256.0 * err, (T, gap, err)


def test_tie_cases_are_exact_ties_across_the_fifth_rank():
    for name, (T, tied, first, picked) in R.PICK_TIES.items():
        sim, strive, part = R.tie_inputs(name)
        for dtype in (F64, torch.float32):
            score, sel, shat, new = R.qam_pick(sim, strive, part, R.TIE_HW, dtype=dtype)
            assert all(torch.equal(score[:, t], score[:, tied[0]]) for t in tied)
            rank = (score > score[:, tied[0]][:, None]).sum(1)             # scores above the tie: the same count in every row
            assert (rank == len(first)).all() and len(first) < 5 < len(first) + len(tied)
            assert sel.tolist() == [list(picked)] * T
            assert R.tie_check(name, score, sel, shat, new).ok
        keep = [t for t in tied if t in picked]
        assert keep == list(tied[:len(keep)]) and len(keep) == 5 - len(first)                  # the lowest indices of the tie


@pytest.mark.parametrize("name", list(R.PICK_WRONG))
def test_pick_wrong_variant_is_caught(name):
    kw = R.PICK_WRONG[name]
    ties = []
    for tie in R.PICK_TIES:
        sim, strive, part = R.tie_inputs(tie)
        k2 = dict(kw, divisor=R.TIE_NBLK * 256) if name == "confidence_over_nblk_256" else kw
        ties.append(R.tie_check(tie, *R.qam_pick(sim, strive, part, R.TIE_HW, **k2)))
    if name == "ties_to_the_highest_index":                               # visible at exact ties only, and at every one of them
        assert all(not c.ok for c in ties)
        return
    runs = _pick_runs(lambda T: [res for _, res in R.pick_sequence(T, **kw)])
    assert any(not c.ok for c in runs), name
    caught = [T for T, c in zip(R.PICK_CASES, runs) if not c.ok]
    assert any(T > 8 for T in caught) and any(T <= 8 for T in caught), (name, caught)


# ------------------------------------------------------------------------------------------------ attention: cases and wrong variants
ATTN_NAMES = ([("table", 32, n, ksel) for n in R.ATTN32_N for ksel in R.ATTN32_KSEL] + [("table", 64, n, ksel) for n in R.ATTN64_N for ksel in R.ATTN64_KSEL]
              + [("sharded", 32), ("sharded", 64), ("fixup",)])


def _attn_runs(fn, names=ATTN_NAMES):
    out = []
    for name in names:
        res = fn(name)
        if res is not None:
            hid, mfg = res
            out += [R.attn_check(name, p, hid, mfg) for p in (0, 1)]
    return out


def _attn_exact(name):
    hid = R.attn_ref(*name)[0].float().to(torch.bfloat16)
    return hid, R.mfg_of(R.attn_named_inputs(*name)[0][5], hid)


def _attn_f32(name):
    (q, k, v, sel, ksel, mf), scale = R.attn_named_inputs(*name)
    hid = R.mem_attn_f32(q, k, v, sel, ksel, scale)
    return hid, R.sp_round(mf + R.ATTN_BETA * hid.float().reshape(mf.shape))


def test_attn_cases_pass_the_reference_and_fp32():
    runs = _attn_runs(_attn_exact) + _attn_runs(_attn_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]


@pytest.mark.parametrize("name", list(R.ATTN_WRONG))
def test_attn_wrong_variant_is_caught(name):
    runs = _attn_runs(lambda case: R.mem_attn_wrong(name, case))
    assert runs and any(not c.ok for c in runs), name
    for kernel in (32, 64):                                                # both kernels' tables see every mistake that applies to them
        mine = [c for c in runs if f"'table', {kernel}" in c.label]
        assert not mine or any(not c.ok for c in mine), (name, kernel)


# ================================================================================================ correlation build, flow output
# ------------------------------------------------------------------------------------------------ references vs torch / the oracle
@pytest.mark.parametrize("case", list(R.CORR_CASES))
def test_corr_pyramid_vs_oracle(case):
    """the float64 pyramid against the oracle's corr_pyramid fed float64 (its einsum runs in fp32: compared at fp32 rounding) and against
    avg_pool2d([1, 2]) of the float64 volume level by level"""
    from oracle import ppm_oracle as O
    B, C, H, W, _ = R.CORR_CASES[case]
    f1, f2 = R.corr_inputs(case)
    got = R.corr_pyramid(f1, f2)
    want = O.corr_pyramid(f1, f2)
    assert len(got) == len(want) == 5
    lvl = got[0].reshape(-1, 1, 1, W)
    for l in range(5):
        assert got[l].shape == (B * H * W, W >> l)
        close(got[l], want[l].reshape(B * H * W, W >> l), 1e-5)
        close(got[l], lvl.reshape(B * H * W, -1))
        lvl = F.avg_pool2d(lvl, [1, 2], stride=[1, 2]) if l < 4 else None
    vol = got[0].reshape(B, H, W, W)
    b, y, i, j = B - 1, H // 2, 3, W - 2
    close(vol[b, y, i, j], (f1[b, :, y, i].double() * f2[b, :, y, j].double()).sum() / math.sqrt(C))
    assert 0.3 < f1.mean() < 0.7 and 0.3 < f2.mean() < 0.7                     # the features' mean is not zero
    s = (f1 - 0.5).std((0, 2, 3))
    assert s.min() < 0.4 and s.max() > 2.5                                     # per-channel scales over 0.25 .. 4


def test_corr_case_arithmetic():
    """which kernel a case runs and what it strains, re-derived from ppms_corr_build's dispatch"""
    line = lambda c: c[3] % 4 == 0 and c[1] % 16 == 0 and not c[4]
    cs = R.CORR_CASES
    assert [k for k in cs if line(cs[k])] == ["w32_c32", "w64_c48", "w128_c16", "w128_c64"]
    assert cs["w32_c32"][3] <= 32 < cs["w64_c48"][3] <= 64 < cs["w128_c16"][3]
    assert [cs[k][1] // 16 for k in cs if line(cs[k])] == [2, 3, 1, 4]                             # nch
    assert [cs["w32_c32"][3] >> l for l in range(1, 5)] == [10, 5, 2, 1] and [cs["w64_c48"][3] >> l for l in range(1, 5)] == [22, 11, 5, 2]
    assert -(-132 // 128) == 2 and 132 - 128 == 4 and -(-260 // 128) == 3
    lines = {k: c[0] * c[2] for k, c in cs.items()}
    assert lines["w32_c32"] == 9 and lines["w128_c64"] == 8 and lines["w128_c16"] == 10 and lines["general_w70"] == 9 and lines["general_c7"] == 8
    assert -(-70 // 32) == 3 and 70 % 4 and 20 % 16 and 7 % 2 and 18 % 4
    for case, (B, C, H, W, mis) in cs.items():                                                     # the layout of the guarded pyramid buffer
        off = 0
        for l in range(5):
            if line(cs[case]):
                assert (off * 4) % (16 if l == 0 else 8 if l == 1 else 4) == 0
            off += B * H * W * (W >> l) + R.CORR_GAPS[l]


@pytest.mark.parametrize("dim,case", [(2, c) for c in R.CONVEX2D_CASES] + [(3, c) for c in R.CONVEX3D_CASES])
def test_convex_upsample_vs_oracle(dim, case):
    """on the cases' own inputs: the 2-D form against the oracle; the 3-D form against the oracle on the extended volume with the mask zero
    outside the own frames, as tests/sharded_oracle.py states it"""
    from oracle import ppm_oracle as O
    flow, mask, th = R.convex_inputs(dim, case, "unit")
    T = mask.shape[0]
    f, m = flow.double().permute(0, 3, 1, 2), mask.double().permute(0, 3, 1, 2)
    if dim == 2:
        close(R.convex_upsample(flow, mask), O.convex_upsample(f, m))
    else:
        m_ext = torch.zeros(T + 2 * th, *m.shape[1:], dtype=F64)
        m_ext[th:th + T] = m
        close(R.convex_upsample_3d(flow, mask, th), O.convex_upsample_3d(f, m_ext, 4, T + 2 * th)[th:th + T])


def test_tap_gather_sum_vs_conv3d():
    """a 3 x 3 x 3 and a 5 x 1 x 3 conv to 3 channels as a 1 x 1 GEMM to taps x cout columns plus the shifted sum, own frames of the halo volume"""
    for k3, th in (((3, 3, 3), 1), ((5, 1, 3), 2), ((1, 3, 3), 0)):
        T, H, W, cin, cout = 2, 4, 5, 6, 3
        ntap, Tf = k3[0] * k3[1] * k3[2], T + 2 * th
        x = hash_normal((Tf, H, W, cin), 70).double()
        wt, bias = hash_normal((cout, cin, *k3), 71).double(), hash_normal((cout,), 72).double()
        y = x.reshape(-1, cin) @ wt.permute(2, 3, 4, 0, 1).reshape(ntap * cout, cin).t()        # column tap cout + c
        want = F.conv3d(x.permute(3, 0, 1, 2)[None], wt, bias, padding=tuple(k // 2 for k in k3))[0].permute(1, 2, 3, 0)[th:th + T]
        got, mag = R.tap_gather_sum(y, bias, cout, k3, T, H, W, th)
        close(got, want.reshape(-1, cout))
        assert (mag >= got.abs() - 1e-12).all()


@pytest.mark.parametrize("case", R.BILINEAR_CASES)
def test_bilinear_taps_vs_interpolate(case):
    """the written-out resize (what the variants are made from) is F.interpolate, both conventions"""
    x = R.bilinear_input(case)
    for align in (False, True):
        close(R.bilinear_taps(x, case[4], case[5], align, -0.5), R.bilinear(x, case[4], case[5], align, -0.5))


def test_transpose_inputs_are_distinct_and_spread():
    shapes = {c[:3] for c in R.TRANSPOSE_CASES + R.TRANSPOSE_F32_SRC_EXTRA} | {R.TRANSPOSE_SP_VIEW[:3]}
    for BT, C, HW in shapes:
        x = R.transpose_input(BT, C, HW)
        n = x.numel()
        assert x.unique().numel() == n and R.sp_round(x).unique().numel() == n and R.sp_split(x)[0].float().unique().numel() > n // 40
        assert x.abs().min() == 2.0 ** -20 and 2.0 ** 18 < x.abs().max() < 2.0 ** 20
    x = R.transpose_input(2, 33, 65)
    assert not torch.equal(R.to_channel_last(x).reshape(2, 65, 33)[0], x[0]) and torch.equal(R.to_channel_last(x).reshape(2, 65, 33)[1, 7, 5], x[1, 5, 7])


# ------------------------------------------------------------------------------------------------ the cases pass the reference and fp32, catch the variants
def _corr_runs(fn):
    return [R.corr_check(case, fn(*R.corr_inputs(case))) for case in R.CORR_CASES]


def test_corr_cases_pass_the_reference_and_fp32():
    runs = _corr_runs(R.corr_pyramid) + _corr_runs(R.corr_pyramid_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]
    print("F32 RATIO corr_build", max(c.worst() for c in _corr_runs(R.corr_pyramid_f32)))


@pytest.mark.parametrize("name", list(R.CORR_WRONG))
def test_corr_wrong_variant_is_caught(name):
    runs = _corr_runs(lambda f1, f2: R.corr_pyramid(f1, f2, **R.CORR_WRONG[name]))
    bad = [c.label.split()[1] for c in runs if not c.ok]
    assert bad, name
    if name != "ceil_widths":                                                  # every case has a full group of 8 lines; ceil: w128_c64's widths are
        assert len(bad) == len(runs), (name, bad)                              # even down to level 2


def _convex_runs(dim, fn):
    """fn(flow, mask, t_halo) over every case and kind of data of the kernel"""
    out = []
    for case in (R.CONVEX3D_CASES if dim == 3 else R.CONVEX2D_CASES):
        for data in R.CONVEX_DATA:
            out.append(R.convex_check(dim, case, data, fn(*R.convex_inputs(dim, case, data))))
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_convex_cases_pass_the_reference_and_fp32(dim):
    kt = 3 if dim == 3 else 1
    runs = _convex_runs(dim, lambda f, m, th: R.convex_upsample_3d(f, m, th, kt=kt))
    f32 = _convex_runs(dim, (lambda f, m, th: R.convex_upsample_3d_f32(f, m, th)) if dim == 3 else (lambda f, m, th: R.convex_upsample_f32(f, m)))
    assert all(c.ok for c in runs + f32), [str(c) for c in runs + f32 if not c.ok]
    print(f"F32 RATIO convex_upsample dim={dim}", max(c.worst() for c in f32))


@pytest.mark.parametrize("dim,name", [(2, n) for n in R.CONVEX_WRONG] + [(3, n) for n in R.CONVEX3D_WRONG])
def test_convex_wrong_variant_is_caught(dim, name):
    kw = R.CONVEX3D_WRONG[name]
    runs = _convex_runs(dim, lambda f, m, th: R.convex_upsample_3d(f, m, th, kt=3 if dim == 3 else 1, **kw))
    bad = {c.label for c in runs if not c.ok}
    assert bad, (dim, name)
    if name == "no_max_subtraction":                                           # only the sharp logits show it, and on every case
        assert all(("sharp" in c.label) == (not c.ok) for c in runs), [str(c) for c in runs]
    if name == "halo_frames_read_as_zero":                                     # only where there is a halo
        assert all((c.label in bad) == (case[3] > 0) for c, case in zip(runs, [k for k in R.CONVEX3D_CASES for _ in R.CONVEX_DATA]))


def _tgs_runs(fn):
    """fn(case) -> (out, accum or None) over the cases"""
    return [R.tgs_check(case, *fn(case)) for case in R.TGS_CASES]


def _tgs_with(case, accum="added", **kw):
    y, bias, acc0 = R.tgs_inputs(case)
    out = R.tap_gather_sum(y, bias, *case[:6], **kw)[0].float()               # what a launch returns: fp32
    return out, None if case[8] is None else (acc0 + out if accum == "added" else out)


def test_tgs_cases_pass_the_reference_and_fp32():
    runs = _tgs_runs(_tgs_with) + _tgs_runs(lambda case: _tgs_with(case, dtype=torch.float32))
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]
    for case in R.TGS_CASES:                                                   # the bound in units of itself: the fp32 form's share of it
        y, bias, _ = R.tgs_inputs(case)
        ref, mag = R.tgs_ref(case)
        ntap = case[1][0] * case[1][1] * case[1][2]
        err = (R.tap_gather_sum_f32(y, bias, *case[:6]).double() - ref).abs() / ((ntap + 1) * 2.0 ** -24 * mag)
        print("F32 RATIO tap_gather_sum", case, err.max().item())
        assert err.max() <= 1.0


@pytest.mark.parametrize("name", list(R.TGS_WRONG))
def test_tgs_wrong_variant_is_caught(name):
    kw = R.TGS_WRONG[name]
    runs = _tgs_runs((lambda case: _tgs_with(case, accum="overwritten")) if kw is None else (lambda case: _tgs_with(case, **kw)))
    assert any(not c.ok for c in runs), name
    if name == "bias_dropped":
        assert all(not c.ok for c in runs)


def _bilinear_runs(fn):
    out = []
    for case in R.BILINEAR_CASES:
        for align in (False, True):
            for mul in R.BILINEAR_MUL:
                got = fn(R.bilinear_input(case), case[4], case[5], align, mul)
                if got is not None:
                    out.append(R.bilinear_check(case, align, mul, got))
    return out


def test_bilinear_cases_pass_the_reference_and_fp32():
    runs = _bilinear_runs(R.bilinear) + _bilinear_runs(R.bilinear_f32)
    assert all(c.ok for c in runs), [str(c) for c in runs if not c.ok]
    print("F32 RATIO bilinear", max(c.worst() for c in _bilinear_runs(R.bilinear_f32)))


@pytest.mark.parametrize("name", list(R.BILINEAR_WRONG))
def test_bilinear_wrong_variant_is_caught(name):
    runs = _bilinear_runs(R.BILINEAR_WRONG[name])
    assert runs and any(not c.ok for c in runs), name
