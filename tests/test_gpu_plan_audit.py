"""GPU: every convolution launch the planner (ppmstereo_amd/convplan.py) makes for the BASELINE geometries, audited one by one against the
float64 reference of tests/conv_audit.py -- the engines' own descriptors (output views at channel offsets, split epilogue halves, hoisted
pre_f32 shares, the grouped zr1_2 launch, lo_zero_from, V^T, the library's K-slice plans), not descriptors built for a test.

Per launch: accuracy on a pixel sample that crosses every tile boundary, no byte written outside the declared outputs, no read/write
overlap, a valid split-bf16 pair (hi = bf16(hi + lo) up to exact ties) for SP outputs, bitwise determinism.  The sensitivity test shows a one-entry bias change is caught and named.
"""
import collections
import gc
import time

import pytest
import torch

import conv_audit as A
from ppmstereo_amd import _lib as L
from ppmstereo_amd import weights as Wm
from ppmstereo_amd.convplan import ConvOp
from ppmstereo_amd.dist import FrameShard

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
SCALES = (("update_block16", 16, 0), ("update_block08", 8, 1), ("update_block04", 4, 2))     # block, map divisor, Attention_qk index


class HaloGeometry:
    """What a ScaleEngine reads from a dist.FrameShard to lay out a rank's window (5 of 40 frames, halo slabs of FrameShard.HALO frames on
    both sides) -- and nothing else: the audit never exchanges data, so any other attribute access is an error."""

    HALO = FrameShard.HALO

    def __init__(self, f=5, world=8, rank=3):
        self.rank, self.world, self.f, self.T = rank, world, f, f * world
        self.lo, self.hi = rank * f, (rank + 1) * f
        self.group, self.force_comm = None, False

    def __getattr__(self, name):
        raise AssertionError(f"the plan audit must not exchange data (FrameShard.{name})")


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd.cnet import Feature
    from ppmstereo_amd.encoder import BasicEncoder
    from ppmstereo_amd.ppmstereo import PPMStereoHotPath
    from ppmstereo_amd.sst import SSTBlock
    hot = {c3: PPMStereoHotPath(use_convex_3d=c3).load_hot_path_weights(Wm.hot_path_weights(use_convex_3d=c3)).to(DEV).eval() for c3 in (False, True)}
    fnet = BasicEncoder(output_dim=256, norm_fn="instance")
    fnet.load_state_dict(Wm.fnet_weights(), strict=True)
    cnet = Feature("tiny", 256)
    cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sst = SSTBlock()
    sst.load_state_dict(Wm.sst_weights(), strict=True)
    return dict(hot=hot, fnet=fnet.to(DEV).eval(), cnet=cnet.to(DEV).eval(), sst=sst.to(DEV).eval())


def _release():
    """Free released engines now: a ScaleEngine sits in reference cycles (bound methods and closures in its launch table), so dropping the
    last reference frees its gigabytes only when the cyclic collector runs."""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()


class Census:
    def __init__(self):
        self.k = collections.OrderedDict()

    def add(self, rep: A.Report):
        c = self.k.setdefault(rep.kernel, collections.Counter())
        c["n"] += 1
        c["sliced"] += rep.sliced
        c["swept"] += rep.swept
        c["halo"] += rep.halo

    def line(self):
        total = sum(c["n"] for c in self.k.values())
        return f"{total} launches: " + ", ".join(f"{k} {c['n']} (sliced {c['sliced']}, swept {c['swept']}, halo'd {c['halo']})" for k, c in sorted(self.k.items()))


def audit_engine(tag: str, eng, census: Census, fails: list, seed: int) -> int:
    ops = A.conv_ops(eng)
    pool = A.Pool(eng)
    present = {id(o) for o in pool.convops}
    assert len(present) == len(ops) and present == {id(o) for o in ops.values()}, \
        f"{tag}: {len(present)} ConvOps in the engine, {len(ops)} listed for the audit"
    wcache = {}
    for i, (name, op) in enumerate(ops.items()):
        rep = A.audit_op(f"{tag}:{name}", op, pool, seed=seed + i, wcache=wcache)
        census.add(rep)
        if rep.failures:
            fails.append(str(rep))
    return len(ops)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_plan_audit(models, geom):
    from ppmstereo_amd.cnet import _CnetEngine
    from ppmstereo_amd.encoder import _FnetEngine
    from ppmstereo_amd.sst import _SstEngine
    name, T, H, W, convex, encoders, sharded = geom
    _release()                      # (also whatever engines earlier test files left to the cyclic collector)
    t0 = time.time()
    census, fails, audited = Census(), [], 0
    dev = torch.device(DEV)
    for c3 in convex:
        hot = models["hot"][c3]
        for blk_name, s, ai in SCALES:
            blk = getattr(hot, blk_name)
            shard = HaloGeometry(f=T) if sharded else None
            eng = blk.engine(T, H // s, W // s, dev, shard=shard)
            assert eng.halo == (FrameShard.HALO if sharded else 0)
            eng.qk_op(hot.att[ai].packed(dev))                   # the q/k projection begin() launches
            audited += audit_engine(f"{name}/{blk_name}{'/convex3d' if c3 else ''}", eng, census, fails, seed=1000 * s + 7 * c3)
            del eng
            blk._engines.clear()
            _release()
    if encoders:
        fnet, cnet, sst = models["fnet"], models["cnet"], models["sst"]
        eng = _FnetEngine(fnet._pack(dev), 2 * T, H, W, dev, 256)          # left + right images in one call (ppmstereo.py:618)
        audited += audit_engine(f"{name}/fnet", eng, census, fails, seed=11)
        del eng
        _release()
        eng = _CnetEngine(cnet._pack(dev), T, H, W, dev)
        audited += audit_engine(f"{name}/cnet", eng, census, fails, seed=12)
        del eng
        _release()
        eng = _SstEngine(sst._pack(dev), sst.time_embed.detach().float()[0], T, H // 16, W // 16, dev)
        audited += audit_engine(f"{name}/sst", eng, census, fails, seed=13)
        del eng
        _release()
    print(f"\ncensus {name} (T = {T}, {H}x{W}{', rank window with halo slabs' if sharded else ''}): {census.line()}  [{time.time() - t0:.1f} s]")
    assert audited == sum(c["n"] for c in census.k.values())
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
        pool = A.Pool(eng)
        rep = A.audit_op("fh2", op, pool, seed=5)
        assert rep.launched and not rep.failures, str(rep)
        rs, errs = A.bind_regions(op.desc, pool)
        assert not errs
        A.fill_storages(pool, rs, op.desc, 5)
        pix = A.pixel_sample(op.desc.T, op.desc.H, op.desc.W, 5, dev)
        amax = A.reference(op.desc, op.version, op.ysweep, pool, rs, pix)["epi[0].out_f32"].abs().max().item()
        k = 7
        bias = next(r for r in rs if r.name == "bias").view(pool)[0].clone()
        bias[k] += 2.0 ** -10 * amax
        d2 = L.Conv.from_buffer_copy(bytes(op.desc))
        d2.bias = bias.data_ptr()
        op2 = ConvOp(d2, op.keep + [bias], op.version, op.wm_hint, nslice=op.nslice, ysweep=op.ysweep, device=dev)
        rep = A.audit_op("fh2 (bias entry 7 perturbed)", op2, A.Pool(eng, extra=[bias]), seed=5, ref_desc=op.desc)
        print(f"\n{rep}")
        assert rep.launched and rep.failures
        assert rep.bad == {"epi[0].out_f32": [k]}, rep.bad
    finally:
        blk._engines.clear()
        _release()
