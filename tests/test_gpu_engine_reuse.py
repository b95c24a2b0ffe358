"""GPU: a used engine must give a fresh engine's bits.

Every engine (ScaleEngine per (block, T, h, w); the fnet, cnet and SST plans) is built once and replayed for every later clip of its geometry.  A
new one is almost all zeros, so the oracle comparisons -- which run on new engines -- cannot see a launch that reads a buffer before this clip wrote
it.  Here the same clip runs on a used engine (and on one whose every non-constant buffer was overwritten with NaN, tests/engine_reuse.py) and on a
new one; both run the same launches on the same inputs, the loop is deterministic (test_cascade_is_bit_stable_over_many_runs), so every comparison
is torch.equal on raw bits.  No tolerance appears anywhere.

Not covered: frame-sharded engines (halo slabs, _xa_halo and the gathered buffers need a process group), poison between the iterations of one clip
(the recurrent state is live there) and poison under a running ClipPipeline (the video and cascade tests cover the pipeline from outside)."""
import pytest
import torch

import engine_reuse as R
from engine_reuse import DEV
from ingest_util import ingest, model, rand_u8  # noqa: F401  (model: the fixture)
from ppmstereo_amd import _lib as L
from ppmstereo_amd.weights import hash_normal, hash_uniform

pytestmark = pytest.mark.gpu

# (block, T, h, w, clip A has a motion hidden state).  Per block: (3, 16, 32) n = 512 -- the 64-query attention kernel and its flags -- and
# (7, 5, 17) n = 85 -- the generic attention path on an odd map, and ksel = 5 < Tg = 7: the usage counter decides picks.  w >= 16 is the lookup's floor.
# (3, 24, 72) on the 1/4-scale block: the plan with K-sliced and y-swept conv_gemm2 launches (docs/LOG_r15.md, geometry small3).
GEOMETRIES = [(tag, *g) for tag in R.BLOCKS for g in ((3, 16, 32, True), (7, 5, 17, False))] + [("update_block04", 3, 24, 72, True)]
IDS = [f"{tag[-2:]}-T{T}-{h}x{w}" for tag, T, h, w, _ in GEOMETRIES]
SEED_A, SEED_B = 131, 977


def dev():
    return torch.device(DEV)


def fresh_pair(blk, T, h, w):
    """Two NEW engines of one geometry (the block's cache may hold used ones from an earlier case: forgotten first; the packed weights stay)."""
    blk.packed(dev())
    blk._engines.clear()
    e0, e1 = blk.engine(T, h, w, dev(), slot=0), blk.engine(T, h, w, dev(), slot=1)
    assert e0 is not e1 and e0.shard is None and blk.engine(T, h, w, dev()) is e0
    return e0, e1


def census(eng):
    """The (3, 24, 72) case must keep meeting the launches it is there for: if the planner ever changes, it fails instead of going blind."""
    ops = eng.conv_ops()
    sliced = sorted(k for k, o in ops.items() if o.nslice > 1)
    with_ws = sorted(k for k, o in ops.items() if o.ws is not None)
    swept = sorted(k for k, o in ops.items() if o.ysweep)
    print(f"\n(3, 24, 72): {len(ops)} conv ops, nslice > 1: {sliced}; workspaces: {len(with_ws)}; y-swept: {swept}")
    assert sliced and with_ws and swept, (sliced, with_ws, swept)


def used_vs_fresh(model, tag, T, h, w, a_mhs, poisoned, skip=()):  # noqa: F811
    """-> (state and health of clip A on the used engine, the same on the new one, the used engine)."""
    e0, e1 = fresh_pair(getattr(model, tag), T, h, w)
    if (T, h, w) == (3, 24, 72):
        census(e0)
    R.dirty(model, tag, e0, T, h, w, SEED_B, a_mhs)
    if poisoned:
        torch.cuda.synchronize()                    # the engine uses side streams
        done = R.poison(e0, R.SCALE_TABLE)
        torch.cuda.synchronize()
        assert {"X", "Hb[0]", "SEL", "ATT_WS", "_FLOW_full", "STRIVE", "_STRIVE_next", "C1", "pyr[0]", "_health"} <= set(done)
        assert any(k.endswith(".ws") for k in done) == any(o.ws is not None for o in e0.conv_family_ops().values() if hasattr(o, "ws"))
    a = R.clip_inputs(T, h, w, SEED_A, a_mhs)
    got = R.run_clip(model, tag, e0, a, skip=skip)
    want = R.run_clip(model, tag, e1, a)
    R.assert_zero(e0, R.SCALE_TABLE)
    assert (want[1]["calls"], want[1]["tiles"] > 0) == ((3, True) if e0.n % 64 == 0 else (0, False)), want[1]      # (counted where the 64-query kernel runs)
    assert torch.isfinite(want[0][-1]["up"]).all() and not R.same(want[0][-1]["flow"], want[0][0]["flow"])
    return got, want, e0


# ------------------------------------------------------------------------------------------------ a. the inventory
def _engines_of(model):  # noqa: F811
    """(label, table, kinds, build() -> engine, clip(engine)) of the six engine classes' instances, each at a small geometry."""
    from ppmstereo_amd.cnet import _CnetEngine
    from ppmstereo_amd.encoder import _FnetEngine
    from ppmstereo_amd.engine import ScaleEngine
    T, h, w = 2, 4, 16                                  # (the 1/16 map of the audited "min" geometry)
    for tag, ai in R.BLOCKS.items():
        blk = getattr(model, tag)
        pk = blk.packed(dev())
        model.att[ai].packed(dev())
        kinds = ("attn",) if pk.attn is not None else ("hoist",)
        yield (tag, R.SCALE_TABLE, kinds, lambda pk=pk: ScaleEngine(pk, T, h, w, dev()),
               lambda e, tag=tag: R.run_clip(model, tag, e, R.clip_inputs(T, h, w, SEED_A, False), iters=2))
    img = hash_uniform((2, 3, 40, 72), 601).to(DEV)
    fpk, cpk = model.fnet._pack(dev()), model.cnet._pack(dev())
    yield "fnet", R.FNET_TABLE, (), lambda: _FnetEngine(fpk, 2, 40, 72, dev(), 256), lambda e: e.run(img)
    img32 = hash_uniform((1, 3, 32, 64), 602).to(DEV)
    yield "cnet", R.CNET_TABLE, (), lambda: _CnetEngine(cpk, 1, 32, 64, dev()), lambda e: e.run(img32)
    f1, f2 = hash_normal((3, 256, 6, 10), 813).to(DEV), hash_normal((3, 256, 6, 10), 823).to(DEV)
    sst = model.sst
    sst._pack(dev())

    def build_sst():
        sst._engines.clear()
        sst(f1, f2, 3)                                  # (the module's own construction: the time embedding resampled to T = 3)
        return next(iter(sst._engines.values()))
    yield "sst", R.SST_TABLE, (), build_sst, lambda e: e.run(f1, f2)


def test_every_engine_buffer_is_classified(model):  # noqa: F811
    """Every device tensor reachable from an engine is in the engine class's table, every table name is found, and CONST entries hold the same bits
    before and after a clip.  Printed, not asserted: the allocator's growth across the construction next to the bytes the walker found."""
    problems = []
    with torch.cuda.device(dev()):
        for label, table, kinds, build, clip in _engines_of(model):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            eng = build()
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
            found = R.buffers(eng)
            own = {n: t for n, t in found.items() if not (R.classify(table, n) == R.CONST and (n.startswith("pk.") or ".keep[" in n))}
            walked = sum(R.nbytes(t) for t in own.values())
            granules = sum((R.nbytes(t) + 511) // 512 * 512 for t in own.values())
            large = sum(R.nbytes(t) >= (1 << 20) for t in own.values())
            print(f"\n{label}: {len(found)} storages ({len(own)} made by the constructor, {large} of 1 MiB or more); allocator growth {grown} B, "
                  f"walker {walked} B, {granules} B in 512-B granules; unexplained {grown - granules} B")
            const = {n: t.clone() for n, t in found.items() if R.classify(table, n) == R.CONST}
            clip(eng)
            clip(eng)
            torch.cuda.synchronize()
            found = R.buffers(eng)
            problems += [f"{label}: {p}" for p in R.check_table(table, found, kinds)]
            problems += [f"{label}: CONST {n} changed" for n, t in const.items() if not R.same(found[n], t)]
            assert const and len(const) < len(found)
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------ b, c. the update blocks' engines
@pytest.mark.parametrize("tag,T,h,w,a_mhs", GEOMETRIES, ids=IDS)
def test_used_scale_engine_equals_fresh(model, tag, T, h, w, a_mhs):  # noqa: F811
    """Slot 0 after the dirtying sequence (engine_reuse.dirty) against the new slot 1: clip A, three iterations, the whole state after every one."""
    got, want, _ = used_vs_fresh(model, tag, T, h, w, a_mhs, poisoned=False)
    assert R.differences(got, want) == []


@pytest.mark.parametrize("tag,T,h,w,a_mhs", GEOMETRIES, ids=IDS)
def test_poisoned_scale_engine_equals_fresh(model, tag, T, h, w, a_mhs):  # noqa: F811
    """The same with every non-constant buffer of slot 0 poisoned behind clip B: NaN where a value stays a value, in-range wrong values where it
    becomes an address (engine_reuse.SCALE_VALUES), finite junk where zero weights meet it."""
    got, want, _ = used_vs_fresh(model, tag, T, h, w, a_mhs, poisoned=True)
    assert R.differences(got, want) == []


# ------------------------------------------------------------------------------------------------ d. the encoders' plans
def _encoder_case(kind, model):  # noqa: F811
    """-> (module, table, geometry of its plan, run on float input, run on bytes through the ingest door (None for the SST block), inputs A / B)."""
    none32, none64 = L.SP(None, None, 32, 32), L.SP(None, None, 64, 64)
    if kind == "fnet":                                  # tests/test_gpu_encoder.py: fnet_odd
        m, hh, ww = model.fnet, 40, 72
        a = [hash_uniform((1, 3, hh, ww), 640).to(DEV), hash_uniform((1, 3, hh, ww), 740).to(DEV)]
        run = lambda x: torch.cat(m(x))
        plan = lambda: m.plan(2, hh, ww, dev())
        view = lambda p: (p.s0_view(), none64)
        table = R.FNET_TABLE
    elif kind == "cnet":                                # tests/test_gpu_cnet.py: cnet_32
        m, hh, ww = model.cnet, 32, 64
        a = [hash_uniform((1, 3, hh, ww), 632).to(DEV)]
        run = lambda x: torch.cat([o.reshape(-1) for o in m(x[0])])
        plan = lambda: m.plan(1, hh, ww, dev())
        view = lambda p: (none32, p.s0_view())
        table = R.CNET_TABLE
    else:                                               # tests/test_gpu_sst.py: sst_T3
        m = model.sst
        a = [hash_normal((3, 256, 6, 10), 813).to(DEV), hash_normal((3, 256, 6, 10), 823).to(DEV)]
        run = lambda x: torch.cat(m(x[0], x[1], 3))
        return m, R.SST_TABLE, lambda: next(iter(m._engines.values())), run, None, a, [-0.5 * t for t in a]
    a8 = [rand_u8((1, 3, hh, ww), 31).to(DEV), rand_u8((1, 3, hh, ww), 32).to(DEV)]

    def run_bytes(x):
        p = plan()
        with torch.cuda.device(dev()):
            ingest(x[0].data_ptr(), x[1].data_ptr(), 3 * hh * ww, 1, hh, ww, 0, 0, hh, ww, *view(p))
            out = p.run_filled()
        return torch.cat([o.reshape(-1) for o in out]) if isinstance(out, tuple) else out
    return m, table, plan, run, (run_bytes, a8, [(255 - t) // 2 for t in a8]), a, [-0.5 * t for t in a]


@pytest.mark.parametrize("kind", ["fnet", "cnet", "sst"])
def test_used_encoder_engine_equals_fresh(model, kind):  # noqa: F811
    """A new module on input A gives R; the same plan after input B (A's complement, scaled) and with everything that is not CONST poisoned -- s0
    included -- must give R again.  fnet and cnet twice: through forward, and through plan().s0_view() + ppms_video_ingest_u8 + run_filled()."""
    m, table, plan, run, door, a, b = _encoder_case(kind, model)
    for fn, xa, xb in [(run, a, b)] + ([door] if door else []):
        m.invalidate()
        want = fn(xa).clone()
        eng = plan()
        other = fn(xb).clone()
        torch.cuda.synchronize()
        done = R.poison(eng, table)
        torch.cuda.synchronize()
        assert plan() is eng and ("s0" in done or "xin" in done) and len(done) > 10
        got = fn(xa)
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and not torch.equal(other, want)
        assert torch.equal(got, want), f"{kind}: {'forward' if fn is run else 'ingest door'}"


# ------------------------------------------------------------------------------------------------ e. a whole video behind other videos
def _invalidate(model):  # noqa: F811
    for m in (model.fnet, model.cnet, model.sst, model.update_block16, model.update_block08, model.update_block04):
        m.invalidate()


def test_a_video_after_other_videos_gives_a_fresh_models_bits(model):  # noqa: F811
    """forward_batch_test on uint8 videos, kernel_size = 4, iters = 6 (3 / 3 / 6 iterations: the two small scales end on parity == 1).  A: 7 frames of
    60 x 250 (several windows of two different T under the ClipPipeline); then B (9 frames of other content), C (92 x 280: the keep-two caches
    evict), A with quantised output planes, A with diagnostics -- and A again must be what the freshly invalidated model gave."""
    from ppmstereo_amd.ppmstereo import OutputSpec, window_plan
    va, vb, vc = rand_u8((7, 2, 3, 60, 250), 41), rand_u8((9, 2, 3, 60, 250), 42), rand_u8((5, 2, 3, 92, 280), 43)
    assert len({stop - start for start, stop, *_ in window_plan(7, 4)}) == 2
    run = lambda v, **kw: model.forward_batch_test({"stereo_video": v}, kernel_size=4, iters=6, **kw)
    _invalidate(model)
    want = run(va)
    _invalidate(model)
    want_redo = run(va, diagnostics=True)["attn_redo"]
    run(vb)
    run(vc)
    run(va, output=OutputSpec(disparity="u16", uncertainty="u8"))
    redo = run(va, diagnostics=True)["attn_redo"]
    got = run(va)
    assert torch.isfinite(want["disparity"]).all() and tuple(want["disparity"].shape) == (7, 1, 60, 250)
    for k in ("disparity", "uncertainties"):
        assert torch.equal(got[k], want[k]), k
    assert want_redo and redo == want_redo


# ------------------------------------------------------------------------------------------------ f. the cascade under the pipeline
def test_cascade_under_the_pipeline_equals_fresh_engines(model):  # noqa: F811
    from ppmstereo_amd.ppmstereo import ClipPipeline
    from ppmstereo_amd.synth import synth_cascade_feats
    T, H, Wd = 3, 64, 256
    fa, fb = ({k: v.to(DEV) for k, v in synth_cascade_feats(T, H, Wd, seed).items()} for seed in (7, 19))
    with torch.cuda.device(dev()):
        pipe = ClipPipeline(dev())
        got = [model.cascade(f, 6, T, test_mode=True, pipeline=pipe) for f in (fa, fb, fa)]
        pipe.wait()
        torch.cuda.synchronize()
        for blk in (model.update_block16, model.update_block08, model.update_block04):
            blk.invalidate()
        want = model.cascade(fa, 6, T, test_mode=True)
        torch.cuda.synchronize()
    for i in (0, 2):
        assert torch.equal(got[i][0], want[0]) and torch.equal(got[i][1], want[1]), f"clip {i}"
    assert torch.isfinite(want[0]).all() and not torch.equal(got[1][0], got[0][0])


# ------------------------------------------------------------------------------------------------ g. the tests above can fail
def test_the_reuse_tests_can_fail(model, monkeypatch):  # noqa: F811
    """Two planted dependences on the previous clip, neither through an index or a coordinate buffer.  (1) begin() leaves the previous clip's usage
    counter in place: the used-engine comparison at T = 7 must differ.  (2) clip A does not load net on slot 0: the poisoned comparison must differ,
    and the flow it returns holds NaN."""
    from ppmstereo_amd.engine import ScaleEngine
    tag, T, h, w, a_mhs = GEOMETRIES[-2]
    assert (tag, T) == ("update_block04", 7)
    begin, planted = ScaleEngine.begin, {"on": None}

    def begin_keeps_the_counter(self, *args):
        before = self.STRIVE.clone()
        begin(self, *args)
        if self is planted["on"]:
            self.STRIVE.copy_(before)
    monkeypatch.setattr(ScaleEngine, "begin", begin_keeps_the_counter)
    e0, e1 = fresh_pair(getattr(model, tag), T, h, w)
    R.dirty(model, tag, e0, T, h, w, SEED_B, a_mhs)
    planted["on"] = e0
    a = R.clip_inputs(T, h, w, SEED_A, a_mhs)
    diff = R.differences(R.run_clip(model, tag, e0, a), R.run_clip(model, tag, e1, a))
    print(f"\nplant 1 (usage counter survives begin): {len(diff)} differences, first {diff[:4]}")
    assert (0, "STRIVE") in diff and any(k in ("flow", "up", "net") for _, k, *_ in diff if isinstance(k, str))
    monkeypatch.setattr(ScaleEngine, "begin", begin)
    got, want, _ = used_vs_fresh(model, tag, T, h, w, a_mhs, poisoned=True, skip=("set_net",))
    diff = R.differences(got, want)
    print(f"plant 2 (net not loaded): {len(diff)} differences, first {diff[:4]}")
    assert (0, "net") in diff and torch.isnan(got[0][-1]["flow"]).any() and torch.isnan(got[0][-1]["up"]).any()
