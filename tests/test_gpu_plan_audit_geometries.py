"""GPU: the plan audit of tests/test_gpu_plan_audit.py at geometries OFF the baseline -- window lengths from 2 to 20 frames and images from 64x256
to 480x640 and 384x1248, whose maps cross the thresholds the planner (ppmstereo_amd/convplan.py) and the library's rating functions decide by:
conv_gemm6's tile fill (none of these maps reaches it, so its convs move to conv_gemm5 with their engine descriptors: GRU / RH epilogues, hoisted
pre_f32 shares, lo_zero_from = 256, split z | r halves, final's 126 + 64 couts over M = 192), conv_gemm5's tile search, conv_gemm2's K-slice
plans 1..8 in both forms, conv_stream's 4096 / 16384 / 32768 pixels and its two tile shapes, gemm1's 16384.

Per launch the five checks of conv_audit.audit_op (accuracy against float64, bytes outside the outputs, overlap, the SP pair, determinism) under
the project's conv bound.  test_census_conditions then asserts, from the audited ConvOps themselves, that the set of geometries really puts every
kernel on the cases named above: should a rating change move a conv elsewhere, that test says which geometry to add, not the audit silently
covering less.  The sensitivity test perturbs one bias entry of a conv_gemm5-planned launch of the VGA geometry.
"""
import time

import pytest
import torch

import conv_audit as A
from ppmstereo_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (T, H, W, encoders too, (world, rank) of a frame-sharded window or None).  H, W: multiples of 32 (what the model pads to), W >= 256.
# The 1/4, 1/8 and 1/16 maps and what they are here for:
GEOMETRIES = {
    "min": (2, 64, 256, True, None),          # 16x64, 8x32, 4x16: H < kh = 5 and T < kt, everything on conv_stream's 32-pixel tiles / gemm1
    "small3": (3, 96, 288, False, None),      # 24x72, 12x36, 6x18: conv_gemm2 s4 / s6 / s8, y-swept s6; conv_stream just above 4096 pixels
    "t4": (4, 256, 352, False, None),         # 64x88, 32x44, 16x22: unsliced y sweep; the 15-tap z/r conv on conv_stream at 1408 pixels
    "t7": (7, 224, 416, False, None),         # 56x104, 28x52, 14x26: three K slices in both forms; conv_gemm5 for the x sweeps only
    "t20": (20, 160, 288, False, None),       # 40x72, 20x36, 10x18: the reference's longest window; conv_gemm5 at 57600 pixels
    "kitti": (2, 384, 1248, True, None),      # 96x312, 48x156, 24x78: wide rows, two frames
    "vga": (5, 480, 640, True, None),         # 120x160, 60x80, 30x40: conv_gemm5 on every conv conv_gemm6 has at the baseline
    "t20_rank": (5, 160, 288, False, (4, 1)),  # frames 5..9 of t20 between halo slabs: conv_stream and K-sliced conv_gemm2 with t_halo
    "vga_rank": (5, 480, 640, False, (4, 1)),  # frames 5..9 of 20 at VGA: conv_gemm5's temporal convs (zr3, fh1, mask_3d.0) with t_halo
}


@pytest.fixture(scope="module")
def models():
    return A.load_models(DEV)


@pytest.fixture(scope="module")
def audits(models):
    """name -> (census, failures, launches, seconds) of a geometry, audited on first use: the census conditions read the launches of the
    geometry cases that ran before them and audit only what has not run yet."""
    done = {}

    def run(name):
        if name not in done:
            T, H, W, encoders, shard = GEOMETRIES[name]
            t0 = time.time()
            census, fails, audited = A.audit_geometry(models, name, T, H, W, (False, True), encoders, shard, DEV)
            done[name] = (census, fails, audited, time.time() - t0)
        return done[name]
    return run


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_plan_audit_geometry(audits, name):
    T, H, W, encoders, shard = GEOMETRIES[name]
    census, fails, audited, secs = audits(name)
    window = f", frames {shard[1] * T}..{shard[1] * T + T - 1} of {shard[0] * T} with halo slabs" if shard else ""
    print(f"\ncensus {name} (T = {T}, {H}x{W}{window}{', with encoders' if encoders else ''}): {census.line()}  [{secs:.1f} s]")
    print(f"plans {name}: {census.plans()}")
    print(f"conv_gemm5 at the 1/4 scale of {name}: {' '.join(census.served('conv_gemm5', 4)) or 'none'}")
    assert not fails, f"{len(fails)} of {audited} launches failed:\n" + "\n".join(fails)


def test_census_conditions(audits):
    """Conditions on the CHOICE of geometries, read from the audited ConvOps: every kernel is launched, with an engine descriptor, on each of
    the cases this file exists for."""
    every = [(g, l) for g in GEOMETRIES for l in audits(g)[0].launches]
    where = lambda **kw: [(g, l) for g, l in every if all(getattr(l, k) == v for k, v in kw.items())]
    missing = []

    def need(what, found):
        if not found:
            missing.append(what)

    # conv_gemm5 at the 1/4 scale: the GRU convs over [h | mf, hid] with the folded weights (lo_zero_from = 256) and their twins over
    # [h | mf, mfg], the W-pass tails, the encoder tail, the heads
    gru = ("zr1_0", "q1", "zr2", "q2", "zr3")
    for conv in [c + "_x" for c in gru] + list(gru) + ["z1_2", "r1_2", "convc2_0", "convc2_1", "final_0", "final_1", "unc0", "fh1"]:
        need(f"conv_gemm5 serving {conv} at the 1/4 scale", where(kernel="conv_gemm5", scale=4, conv=conv))
    for c3 in (False, True):
        need(f"conv_gemm5 serving m1 at the 1/4 scale, use_convex_3d = {c3}", where(kernel="conv_gemm5", scale=4, conv="m1", convex3d=c3))
    # (z1_2 and r1_2 as two launches: the grouped zr1_2 launch is conv_gemm6's alone and must not be planned next to them)
    engines = lambda **kw: {(g, l.convex3d) for g, l in where(scale=4, **kw)}
    need("z1_2 and r1_2 on conv_gemm5 in an engine without the grouped zr1_2 launch",
         (engines(kernel="conv_gemm5", conv="z1_2") & engines(kernel="conv_gemm5", conv="r1_2")) - engines(conv="zr1_2"))
    # conv_gemm2: every K-slice plan of the library, in both forms
    plain = {l.nslice for g, l in where(kernel="conv_gemm2", ysweep=False)}
    swept = {l.nslice for g, l in where(kernel="conv_gemm2", ysweep=True)}
    need(f"plain conv_gemm2 with 2, 3, 4, 6 and 8 K slices (found {sorted(plain)})", plain >= {2, 3, 4, 6, 8})
    need(f"y-swept conv_gemm2 with 1, 2, 4 and 6 K slices (found {sorted(swept)})", swept >= {1, 2, 4, 6})
    # conv_stream: above 4096 pixels its rating (ppms_conv_stream_applicable) keeps only convs without spatial taps and 64-cout convs, so the
    # wide 3x3 conv and the 15-tap conv can only be met below; the temporal conv and the 64-cout 3x3 conv on both sides.  32-pixel tiles:
    # <= 4096 pixels and fewer than 192 padded rows; 64-pixel tiles: everything else.
    stream = [l for g, l in where(kernel="conv_stream")]
    need("conv_stream serving a 3x3 conv with >= 192 couts", [l for l in stream if l.taps == (1, 3, 3) and l.couts >= 192])
    need("conv_stream serving the 15-tap zr1_0", [l for l in stream if l.conv.startswith("zr1_0") and l.taps == (1, 1, 15)])
    for side, big in (("<= 4096", False), ("> 4096", True)):
        need(f"conv_stream with P {side}", [l for l in stream if (l.pixels > 4096) == big])
        need(f"conv_stream serving a temporal (5, 1, 1) conv with P {side}", [l for l in stream if l.taps == (5, 1, 1) and (l.pixels > 4096) == big])
        need(f"conv_stream serving a 64-cout 3x3 conv with P {side}", [l for l in stream if l.taps == (1, 3, 3) and l.couts == 64 and (l.pixels > 4096) == big])
    need("conv_stream on 32-pixel tiles with 128 couts", [l for l in stream if l.pixels <= 4096 and l.couts == 128])
    # gemm1
    gemm1 = [l for g, l in where(kernel="gemm1")]
    need("gemm1 serving to_v with out_vt", [l for l in gemm1 if l.conv == "to_v" and l.vt])
    need("gemm1 serving m2", [l for l in gemm1 if l.conv == "m2"])
    need("gemm1 serving sa_qkv", [l for l in gemm1 if l.conv == "sa_qkv"])
    for side, small in (("<= 4096", True), ("> 4096", False)):
        need(f"gemm1 with P {side}", [l for l in gemm1 if (l.pixels <= 4096) == small])
    # temporal taps that read the halo slabs of a sharded window
    for kernel in ("conv_gemm5", "conv_gemm2", "conv_stream"):
        need(f"{kernel} serving a temporal-tap conv with t_halo > 0", [l for g, l in where(kernel=kernel, halo=True) if l.taps[0] > 1])
    total = len(every)
    secs = sum(audits(g)[3] for g in GEOMETRIES)
    worst = {}
    for g, l in every:
        worst[l.kernel] = max(worst.get(l.kernel, 0.0), l.worst)
    print(f"\n{total} launches over {len(GEOMETRIES)} geometries in {secs:.1f} s; worst max-error / bound per kernel: " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not missing, "the geometries no longer cover:\n" + "\n".join(missing)


def test_geometry_audit_catches_one_bias_entry(models):
    """The new coverage bites: zr1_0_x of the VGA geometry's 1/4 scale on conv_gemm5 (GELU halves z | r split at 128, the hoisted pre_f32
    share, lo_zero_from = 256).  With entry 133 of a test-owned bias copy off by 2^-10 max |ref| the audit, comparing against the reference
    of the original bias, must fail and name exactly cout 5 of the second half."""
    T, H, W = GEOMETRIES["vga"][:3]
    blk = models["hot"][False].update_block04
    eng = blk.engine(T, H // 4, W // 4, torch.device(DEV))
    try:
        op = eng.op["zr1_0_x"]
        d = op.desc
        assert A.kernel_name(op) == "conv_gemm5" and (d.M, d.m_split, d.lo_zero_from) == (256, 128, 256)
        assert all(d.epi[h].kind == L.EPI_STORE and d.epi[h].act == L.ACT_GELU and d.epi[h].pre_f32 and d.epi[h].n_valid == 128 for h in (0, 1))
        rep = A.audit_with_bias_entry_off("vga/update_block04:zr1_0_x", op, eng, 133, "epi[1].out_sp", seed=5)
        print(f"\n{rep}")
        assert rep.launched and rep.failures
        assert rep.bad == {"epi[1].out_sp": [5]}, rep.bad
    finally:
        blk._engines.clear()
        A.release()
