"""GPU: every convolution launch the planner (ppmstereo_amd/convplan.py) makes for the BASELINE geometries, audited one by one against the
float64 reference of tests/conv_audit.py -- the engines' own descriptors (output views at channel offsets, split epilogue halves, hoisted
pre_f32 shares, the grouped zr1_2 launch, lo_zero_from, V^T, the library's K-slice plans), not descriptors built for a test.

Per launch: accuracy on a pixel sample that crosses every tile boundary, no byte written outside the declared outputs, no read/write
overlap, a valid split-bf16 pair (hi = bf16(hi + lo) up to exact ties) for SP outputs, bitwise determinism.  The sensitivity test shows a one-entry bias change is caught and named.
"""
import time

import pytest
import torch

import conv_audit as A
from ppmstereo_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, T, H, W, use_convex_3d variants, encoders too, sharded window)
GEOMETRIES = [
    ("config2", 5, 320, 512, (False, True), True, False),
    ("config3", 5, 736, 1280, (False, True), True, False),
    ("config4_T40", 40, 320, 512, (False, True), False, False),
    ("config5_T40", 40, 736, 1280, (False, True), False, False),
    ("config4_rank_window", 5, 320, 512, (False, True), False, True),
    ("config5_rank_window", 5, 736, 1280, (False, True), False, True),
]


@pytest.fixture(scope="module")
def models():
    return A.load_models(DEV)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_plan_audit(models, geom):
    name, T, H, W, convex, encoders, sharded = geom
    t0 = time.time()
    census, fails, audited = A.audit_geometry(models, name, T, H, W, convex, encoders, (8, 3) if sharded else None, DEV)     # rank 3 of 8: frames 15..19 of 40
    print(f"\ncensus {name} (T = {T}, {H}x{W}{', rank window with halo slabs' if sharded else ''}): {census.line()}  [{time.time() - t0:.1f} s]")
    assert not fails, f"{len(fails)} of {audited} launches failed:\n" + "\n".join(fails)


def test_plan_audit_catches_one_bias_entry(models):
    """One launch with a test-owned bias copy whose entry k is off by 2^-10 max|ref| (an in-bounds descriptor): the audit, comparing against
    the reference of the original bias, must fail and name exactly cout k."""
    dev = torch.device(DEV)
    blk = models["hot"][False].update_block08
    eng = blk.engine(5, 40, 64, dev)
    try:
        op = eng.op["fh2"]
        e = op.desc.epi[0]
        assert e.kind == L.EPI_STORE and e.act == L.ACT_NONE and e.scale == 1.0 and not e.pre_f32 and e.out_f32
        k = 7
        rep = A.audit_with_bias_entry_off("fh2", op, eng, k, "epi[0].out_f32", seed=5)
        print(f"\n{rep}")
        assert rep.launched and rep.failures
        assert rep.bad == {"epi[0].out_f32": [k]}, rep.bad
    finally:
        blk._engines.clear()
        A.release()
