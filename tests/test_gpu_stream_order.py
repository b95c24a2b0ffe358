"""GPU: every hand-off between two streams must hold with either stream held back.

The hot path hands work from stream to stream in five places: the branches of an iteration (ScaleEngine._fork / _join, stream _side), the hoisted
gate pre-activations (set_inp -> _pre_stream -> update()), consecutive clips (ClipPipeline.small / .large), cnet beside fnet (the encoder stream)
and the allocator's lifetimes (record_stream).  At natural timing a missing wait is invisible: the consumer's launch lands behind the producer's
anyway, and a read that comes too early finds the previous, often identical, answer.  Here one role at a time is held back (tests/stream_hold.py:
a delay behind every synchronisation call the role's streams make), consecutive clips differ, scratch is poisoned (tests/engine_reuse.py) -- and
every result must be the bits of the same case with nothing held.  No tolerance appears anywhere.

The delay is measured, not chosen: 1.5 x the event-timed duration of the unheld case (median of 3 after a warm-up), so that a held segment
starts after everything the other streams can do without it has been done.  The three plants of the last two tests are the check that it is long
enough.  A process has fewer hardware queues than these cases have streams, and a delay also holds back what shares the held stream's queue: that
can hide a difference and never invent one.  The one-engine case and the pipeline's plant place their streams by measurement first (EngineCase.alone,
CascadeCase.large_holds_nobody_else); the other runs keep the placement they get.

Not covered: frame-sharded engines (their halo and gather handles hand off to the communication library's own stream, which these hooks do not
see, and need a process group); host-side races other than those the cases cross."""
import contextlib
import time

import pytest
import torch

import engine_reuse as R
import stream_hold as H
from engine_reuse import DEV
from ingest_util import model, rand_u8  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 131, 977
FACTOR = 1.5                                            # delay = FACTOR x the unheld duration of the case
TAGS = ("update_block16", "update_block08", "update_block04")


def dev():
    return torch.device(DEV)


@pytest.fixture(scope="module")
def timing():
    """The delay's calibration, once; the cases keep their unheld durations on their own objects."""
    with torch.cuda.device(dev()):
        d = H.calibrate()
    print("\n" + "\n".join(d.report))
    return d


def engine_roles(roles, blk_tag, eng):
    roles.add(f"side:{blk_tag}", eng._side)
    if eng.pk.hoist:
        roles.add(f"pre:{blk_tag}", eng._pre_stream)


def held_run(label, role, roles, delay, run, prepare=None):
    """prepare(), then run() under the hooks with ``role`` held -> (result, ledger); the census of the run is asserted and printed."""
    if prepare is not None:
        prepare()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with H.hold(role, roles, delay if role is not None else 0) as ledger:
        got = run()
    wall = time.perf_counter() - t0
    print(f"\n[{label}] held: {role}, delay {delay if role is not None else 0:.2f} ms x {ledger.delays[role] if role else 0}, wall {wall * 1e3:.0f} ms\n{ledger.table()}")
    silent = [r for r in roles.names() if r not in ledger.roles()]
    assert not silent, f"{label}: no synchronisation call by {silent}"
    assert role is None or ledger.delays[role] >= 1
    return got, ledger


def unheld(label, roles, run, prepare=None):
    """-> (delay, reference result, reference ledger): the unheld duration with events, and the reference run under the hooks with no delay."""
    ms, runs = H.time_ms(run, prepare)
    print(f"\n[{label}] unheld {ms:.3f} ms (runs {[round(x, 3) for x in runs]}) -> delay {FACTOR * ms:.3f} ms")
    want, ledger = held_run(label, None, roles, 0.0, run, prepare)
    return FACTOR * ms, want, ledger


# ------------------------------------------------------------------------------------------------ a. one engine, one clip
# (block, T, h, w, clip A has a motion hidden state): update_block16 at n = 512 (the 64-query attention and its fix-up); the hoisted blocks there
# and on an odd map (generic paths)
ENGINE_CASES = [("update_block16", 3, 16, 32, True)] + [(tag, *g) for tag in TAGS[1:] for g in ((3, 16, 32, True), (7, 5, 17, False))]
ENGINE_IDS = [f"{tag[-2:]}-T{T}-{h}x{w}" for tag, T, h, w, _ in ENGINE_CASES]


class EngineCase:
    """A NEW engine of the geometry (slot 0; the block's cache is forgotten first, so that its streams are drawn from the pool in one go), clip A,
    and the preparation of engine_reuse.dirty: clip B, then the poison."""

    def __init__(self, model, tag, T, h, w, a_mhs):  # noqa: F811
        self.model, self.tag, self.geom, self.a_mhs = model, tag, (T, h, w), a_mhs
        blk = getattr(model, tag)
        blk.packed(dev())
        blk._engines.clear()
        with torch.cuda.device(dev()):
            self.eng = blk.engine(T, h, w, dev())
            self.default = torch.cuda.current_stream()
        self.attrs = {f"side:{tag}": "_side", **({f"pre:{tag}": "_pre_stream"} if self.eng.pk.hoist else {})}
        self.roles = self.role_map()
        self.a = R.clip_inputs(T, h, w, SEED_A, a_mhs)
        self.label = f"a {tag} {self.geom}"

    def streams(self):
        return {"caller": self.default, **{name: getattr(self.eng, attr) for name, attr in self.attrs.items()}}

    def role_map(self):
        roles = H.RoleMap()
        for name, stream in self.streams().items():
            roles.add(name, stream)
        return roles

    @contextlib.contextmanager
    def alone(self, role):
        """-> the role map, with the held role's stream on a hardware queue that no other stream of the case shares.  A process has a few hardware
        queues, each worked off in order, and torch's streams are spread over them: a delay on the held stream also holds back whatever shares
        its queue, and then nothing can run ahead of it and a missing wait stays hidden (seen with plant 2 in a process that had run the rest of
        the suite).  So a side or pre-activation stream that holds another stream of the case back (stream_hold.blocks: measured) is replaced by
        one of the pool that does not -- the streams are plain attributes of the engine, read at every call -- and with the caller's stream held
        the two others are replaced if it holds them back."""
        saved = []

        def replace(name, ok):
            for _ in range(32):
                s = torch.cuda.Stream(device=dev())
                if s.cuda_stream not in {x.cuda_stream for x in self.streams().values()} and ok(s):
                    saved.append((self.attrs[name], getattr(self.eng, self.attrs[name])))
                    setattr(self.eng, self.attrs[name], s)
                    return
            raise AssertionError(f"{name}: every stream of the pool shares a hardware queue with another stream of the case")
        try:
            with torch.cuda.device(dev()):
                if role == "caller":
                    for name in self.attrs:
                        if H.blocks(self.default, self.streams()[name]):
                            replace(name, lambda s: not H.blocks(self.default, s))
                elif role is not None:
                    others = [s for name, s in self.streams().items() if name != role]
                    if any(H.blocks(self.streams()[role], o) for o in others):
                        replace(role, lambda s: not any(H.blocks(s, o) for o in others))
            if saved:
                print(f"\n[{self.label}] {role} held: {len(saved)} stream(s) replaced so that it has a hardware queue of its own")
            yield self.role_map()
        finally:
            torch.cuda.synchronize()
            for attr, stream in saved:
                setattr(self.eng, attr, stream)

    def prepare(self):
        R.dirty(self.model, self.tag, self.eng, *self.geom, SEED_B, self.a_mhs)
        torch.cuda.synchronize()
        R.poison(self.eng, R.SCALE_TABLE)
        torch.cuda.synchronize()

    def run(self):
        return R.run_clip(self.model, self.tag, self.eng, self.a)


@pytest.mark.parametrize("tag,T,h,w,a_mhs", ENGINE_CASES, ids=ENGINE_IDS)
def test_one_engine_with_each_stream_held(model, timing, tag, T, h, w, a_mhs):  # noqa: F811
    """Clip A, three iterations, on a used and poisoned engine: the whole state after every iteration with the caller's stream, the side stream
    and (hoisted blocks) the pre-activation stream held in turn, against the run with nothing held."""
    case = EngineCase(model, tag, T, h, w, a_mhs)
    delay, want, ref = unheld(case.label, case.roles, case.run, case.prepare)
    assert torch.isfinite(want[0][-1]["up"]).all() and not R.same(want[0][-1]["flow"], want[0][0]["flow"])
    assert case.roles.names() == sorted(["caller", f"side:{tag}"] + ([f"pre:{tag}"] if tag != "update_block16" else []))
    for role in case.roles.names():
        with case.alone(role) as roles:
            got, ledger = held_run(case.label, role, roles, delay, case.run, case.prepare)
        assert ledger.counts == ref.counts, f"{role} held: another path was taken"
        assert R.differences(got, want) == [], f"{role} held"


# ------------------------------------------------------------------------------------------------ b, d. the cascade under a ClipPipeline
class CascadeCase:
    """[A, B, A] at (3, 64, 256), iters = 4, through ONE ClipPipeline, enqueued and collected as forward_batch_test does: clip k + 1 is enqueued
    before clip k's result is waited for (``wait(handle)``) and read on the caller's stream.  Every clip's inputs are copies made on the caller's
    stream inside the run (so the hand-off of the inputs is in play) and dropped behind the call (so the allocator's is).  The three engines are
    poisoned in front of every run."""
    T, H, W, ITERS = 3, 64, 256, 4

    def __init__(self, model):  # noqa: F811
        from ppmstereo_amd.ppmstereo import ClipPipeline
        from ppmstereo_amd.synth import synth_cascade_feats
        self.model = model
        self.fa, self.fb = ({k: v.to(DEV) for k, v in synth_cascade_feats(self.T, self.H, self.W, seed).items()} for seed in (7, 19))
        for tag in TAGS:                                # new engines, the pipeline and the caller's own stream: drawn from the pool in one go
            getattr(model, tag).invalidate()
        with torch.cuda.device(dev()):
            model.cascade(self.fa, self.ITERS, self.T, test_mode=True)
            torch.cuda.synchronize()
            self.pipe = ClipPipeline(dev())
            self.own = torch.cuda.Stream(device=dev())
            self.default = torch.cuda.current_stream()
        self.engines = {tag: self.engine(tag) for tag in TAGS}
        self.measured = {}                              # (variant, caller) -> (delay, reference results, reference ledger)
        self.plain = {}                                 # variant -> results of cascade without a pipeline, for A and for B

    def engine(self, tag):
        engs = list(getattr(self.model, tag)._engines.values())
        return engs[0] if len(engs) == 1 else None

    def current(self):
        return all(self.engine(tag) is e for tag, e in self.engines.items())

    def roles(self, own_stream):
        roles = H.RoleMap().add("caller", self.own if own_stream else self.default).add("pipe.small", self.pipe.small).add("pipe.large", self.pipe.large)
        for tag, eng in self.engines.items():
            engine_roles(roles, tag, eng)
        return roles

    def prepare(self):
        torch.cuda.synchronize()
        for eng in self.engines.values():
            R.poison(eng, R.SCALE_TABLE)
        torch.cuda.synchronize()

    def small_side(self):
        """name -> (owner, attribute) of every stream the small scales of the NEXT clip run on while large is in front of this clip's prologue."""
        e16, e08 = self.engines["update_block16"], self.engines["update_block08"]
        return {"pipe.small": (self.pipe, "small"), "side:update_block16": (e16, "_side"), "side:update_block08": (e08, "_side"),
                "pre:update_block08": (e08, "_pre_stream")}

    def large_side(self):
        """name -> (owner, attribute) of the streams that wait for large's events all through the 1/4 scale."""
        e04 = self.engines["update_block04"]
        return {"side:update_block04": (e04, "_side"), "pre:update_block04": (e04, "_pre_stream")}

    @contextlib.contextmanager
    def large_holds_nobody_else(self):
        """The streams of a process share a few hardware queues, each worked off in order.  A delay on large therefore also delays whatever shares
        its queue -- and the 1/4 engine's side and pre-activation streams, which wait for large's events from the first set_inp on, block whatever
        shares THEIR queues.  If any of that is a stream of ``small_side`` (or the caller's), the next clip cannot run ahead of a held large and
        a missing wait between the two stages stays hidden.  Inside this context the 1/4 scale's three streams lie on one hardware queue and
        nothing else of the case does: streams are replaced by streams of the pool until a spin on large holds back exactly those it should
        (stream_hold.blocks: measured, not assumed; the streams are plain attributes of the pipeline and the engines, read at every call).
        -> [(name, pool streams tried)] of what was replaced."""
        saved, notes = [(self.pipe, "large", self.pipe.large)], []
        taken = set(self.roles(False)) | {self.own.cuda_stream}

        def pool_stream(ok, name):
            for tried in range(1, 33):
                s = torch.cuda.Stream(device=dev())
                if s.cuda_stream not in taken and ok(s):
                    taken.add(s.cuda_stream)
                    notes.append((name, tried))
                    return s
            raise AssertionError(f"{name}: no stream of the pool is free of large's hardware queue")
        try:
            with torch.cuda.device(dev()):
                if H.blocks(self.pipe.large, self.default):
                    self.pipe.large = pool_stream(lambda s: not H.blocks(s, self.default), "pipe.large")
                for group, shares in ((self.small_side(), False), (self.large_side(), True)):
                    for name, (owner, attr) in group.items():
                        if H.blocks(self.pipe.large, getattr(owner, attr)) != shares:
                            saved.append((owner, attr, getattr(owner, attr)))
                            setattr(owner, attr, pool_stream(lambda s: H.blocks(self.pipe.large, s) == shares, name))
            yield notes
        finally:
            torch.cuda.synchronize()
            for owner, attr, stream in saved:
                setattr(owner, attr, stream)

    def kwargs(self, variant):
        from ppmstereo_amd.output import OutputSpec, _EgressCall
        kw = {}
        if variant == "diagnostics":
            kw["diagnostics"] = {}
        if variant == "egress":
            kw["egress"] = _EgressCall(OutputSpec(disparity="u16", uncertainty="u8"))
        return kw

    @staticmethod
    def tensors(result):
        return list(result.values()) if isinstance(result, dict) else list(result)

    def run(self, variant="plain", plant=False):
        """-> [([tensors], attn_redo or None)] of the three clips.  plant: ``pipeline.consumed`` is forgotten before every call (plant 3)."""
        out, pending = [], None

        def collect(result, handle, kw):
            self.pipe.wait(handle)
            out.append(([t.clone() for t in self.tensors(result)], kw.get("diagnostics", {}).get("attn_redo")))
        with torch.cuda.device(dev()):
            for f in (self.fa, self.fb, self.fa):
                kw = self.kwargs(variant)
                if plant:
                    self.pipe.consumed = None
                feats = {k: v.clone() for k, v in f.items()}
                item = (self.model.cascade(feats, self.ITERS, self.T, test_mode=True, pipeline=self.pipe, **kw), self.pipe.last, kw)
                del feats
                if pending is not None:
                    collect(*pending)
                pending = item
            collect(*pending)
            torch.cuda.synchronize()
        return out

    def without_pipeline(self, variant):
        if variant not in self.plain:
            self.prepare()
            res = []
            with torch.cuda.device(dev()):
                for f in (self.fa, self.fb):
                    kw = self.kwargs(variant)
                    r = self.model.cascade(f, self.ITERS, self.T, test_mode=True, **kw)
                    torch.cuda.synchronize()
                    res.append(([t.clone() for t in self.tensors(r)], kw.get("diagnostics", {}).get("attn_redo")))
            self.plain[variant] = res
        return self.plain[variant]

    def reference(self, variant, own_stream=False):
        key = (variant, own_stream)
        if key not in self.measured:
            self.measured[key] = unheld(f"{'d' if own_stream else 'b'} cascade {variant}", self.roles(own_stream), lambda: self.run(variant), self.prepare)
        return self.measured[key]

    @staticmethod
    def compare(got, want):
        """[(clip, index of the tensor, or "attn_redo")] of what differs."""
        bad = [(i, j) for i, (g, w) in enumerate(zip(got, want)) for j, (a, b) in enumerate(zip(g[0], w[0])) if not R.same(a, b)]
        return bad + [(i, "attn_redo") for i, (g, w) in enumerate(zip(got, want)) if g[1] != w[1]] + ([("clips", len(got), len(want))] if len(got) != len(want) else [])


_CASCADE = []


def the_cascade_case(model):  # noqa: F811
    """One CascadeCase for the module, rebuilt if another test has replaced the engines it listed (their streams would be in no role)."""
    if not _CASCADE or _CASCADE[0].model is not model or not _CASCADE[0].current():
        _CASCADE[:] = [CascadeCase(model)]
    return _CASCADE[0]


@pytest.fixture
def cascade_case(model):  # noqa: F811
    return the_cascade_case(model)


def check_cascade(case, variant, role, own_stream=False, plant=False):
    delay, want, ref = case.reference(variant, own_stream)
    plain = case.without_pipeline(variant)
    assert case.compare(want, [plain[0], plain[1], plain[0]]) == [], "the unheld pipelined run against cascade without a pipeline"
    assert all(torch.isfinite(t).all() for t in want[0][0] if t.is_floating_point()) and not R.same(want[1][0][0], want[0][0][0])
    if role is None:
        return want
    got, ledger = held_run(f"{'d' if own_stream else 'b'} cascade {variant}", role, case.roles(own_stream), delay, lambda: case.run(variant, plant), case.prepare)
    if not plant:
        assert ledger.counts == ref.counts, f"{role} held: another path was taken"
        assert case.compare(got, want) == [], f"{role} held"
    return got


CASCADE_ROLES = ["caller", "pipe.small", "pipe.large"] + [f"side:{t}" for t in TAGS] + [f"pre:{t}" for t in TAGS[1:]]


@pytest.mark.parametrize("role", CASCADE_ROLES)
def test_cascade_under_the_pipeline_with_each_stream_held(cascade_case, timing, role):
    """All three results, with every role of the case held in turn, against the unheld pipelined run -- which equals cascade without a pipeline."""
    assert cascade_case.roles(False).names() == sorted(CASCADE_ROLES)
    check_cascade(cascade_case, "plain", role)


@pytest.mark.parametrize("role", ["caller", "pipe.small", "pipe.large"])
def test_cascade_diagnostics_cross_the_streams(cascade_case, timing, role):
    """diagnostics= on: the health snapshots are taken on small and large and read on the caller's stream in wait(handle)."""
    want = check_cascade(cascade_case, "diagnostics", None)
    assert all(redo and set(redo) == {"1/16", "1/8", "1/4"} for _, redo in want)
    check_cascade(cascade_case, "diagnostics", role)


@pytest.mark.parametrize("role", ["caller", "pipe.large"])
def test_cascade_output_planes_cross_the_streams(cascade_case, timing, role):
    """An OutputSpec egress: the planes are allocated and written on large and read on the caller's stream after wait(handle)."""
    want = check_cascade(cascade_case, "egress", None)
    assert [t.element_size() for t in want[0][0]] == [2, 1]
    check_cascade(cascade_case, "egress", role)


@pytest.mark.parametrize("role", [None, "caller"])
def test_cascade_from_a_stream_the_caller_made(cascade_case, timing, role):
    """The library called inside ``with torch.cuda.stream(torch.cuda.Stream())``: unheld and with that stream held, the default stream's bits."""
    want = check_cascade(cascade_case, "plain", None)
    with torch.cuda.device(dev()), torch.cuda.stream(cascade_case.own):
        got = check_cascade(cascade_case, "plain", role, own_stream=True)
    assert cascade_case.compare(got, want) == [], "a caller-made stream against the default stream"


# ------------------------------------------------------------------------------------------------ c. the whole call
class VideoCase:
    """forward_batch_test on the uint8 60 x 250, 7-frame video, kernel_size = 4, iters = 4: two windows (T = 4, T = 3), the ingest kernel, cnet on
    the encoder stream, a ClipPipeline -- after a video of another size, so that the allocator's pools are warm.  forward_batch_test makes a new
    ClipPipeline per call; here every call's pipeline gets the same two streams, so that they can have a role."""

    def __init__(self, model):  # noqa: F811
        self.model = model
        self.va, vc = rand_u8((7, 2, 3, 60, 250), 41), rand_u8((5, 2, 3, 92, 280), 43)
        for m in (model.fnet, model.cnet, model.sst, *(getattr(model, t) for t in TAGS)):
            m.invalidate()
        model.forward_batch_test({"stereo_video": vc}, kernel_size=4, iters=4)
        model._enc_streams.clear()                      # the encoder stream, the pipeline's and the engines': drawn from the pool in one go
        with torch.cuda.device(dev()):
            self.streams = (torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev()))
            self.default = torch.cuda.current_stream()
        self.run()                                      # the unheld warm-up call that creates the engines of A and the encoder stream
        self.engines = self.scale_engines()
        roles = H.RoleMap().add("caller", self.default).add("pipe.small", self.streams[0]).add("pipe.large", self.streams[1])
        roles.add("enc.side", model._enc_streams[dev().index or 0])
        for tag, engs in self.engines.items():
            for eng in engs:
                engine_roles(roles, tag, eng)
        self.roles = roles
        self.measured = None

    def scale_engines(self):
        return {tag: list(getattr(self.model, tag)._engines.values()) for tag in TAGS}

    def current(self):
        return all(len(a) == len(b) and all(x is y for x, y in zip(a, b)) for a, b in zip(self.engines.values(), self.scale_engines().values()))

    @contextlib.contextmanager
    def one_pipeline(self):
        from ppmstereo_amd import ppmstereo as P
        small, large = self.streams
        real = P.ClipPipeline

        class SameStreams(real):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                self.small, self.large = small, large
        P.ClipPipeline = SameStreams
        try:
            yield
        finally:
            P.ClipPipeline = real

    def prepare(self):
        torch.cuda.synchronize()
        for engs in self.engines.values():
            for eng in engs:
                R.poison(eng, R.SCALE_TABLE)
        for eng in self.model.sst._engines.values():
            R.poison(eng, R.SST_TABLE)
        torch.cuda.synchronize()

    def run(self):
        with self.one_pipeline():
            out = self.model.forward_batch_test({"stereo_video": self.va}, kernel_size=4, iters=4)
        torch.cuda.synchronize()
        return out

    def reference(self):
        if self.measured is None:
            self.measured = unheld("c video", self.roles, self.run, self.prepare)
        return self.measured


_VIDEO = []


@pytest.mark.parametrize("role", ["caller", "enc.side", "pipe.small", "pipe.large"])
def test_whole_call_with_each_stream_held(model, timing, role):  # noqa: F811
    from ppmstereo_amd.ppmstereo import window_plan
    if not _VIDEO or _VIDEO[0].model is not model or not _VIDEO[0].current():
        _VIDEO[:] = [VideoCase(model)]
    case = _VIDEO[0]
    assert len({stop - start for start, stop, *_ in window_plan(7, 4)}) == 2
    delay, want, ref = case.reference()
    assert torch.isfinite(want["disparity"]).all() and tuple(want["disparity"].shape) == (7, 1, 60, 250)
    got, ledger = held_run("c video", role, case.roles, delay, case.run, case.prepare)
    assert ledger.counts == ref.counts, f"{role} held: another path was taken"
    for k in ("disparity", "uncertainties"):
        assert torch.equal(got[k], want[k]), f"{role} held: {k}"


# ------------------------------------------------------------------------------------------------ e. the tests above can fail
# Three planted missing waits, each a patch made here and none in the package; each must make the named held run differ from the unheld one, in ONE
# run.  The waits removed order kernels that move values only -- gate activations and the flow branch (1), hoisted pre-activations (2), the 1/8
# engine's flow, hidden state and motion hidden state (3) -- no index or coordinate buffer is written on the stream whose wait goes away
# (engine_reuse.SCALE_VALUES: SEL, ATT_WS and _health are written and read on the caller's stream throughout; the flow is a sampling coordinate only
# for corr_lookup, whose taps take NaN and far positions as "outside").  The unheld run with the plant in place is recorded too: it is expected --
# not required -- to pass, which is the point of this file.
def test_the_engine_tests_can_fail(model, timing, monkeypatch):  # noqa: F811
    """Case (a), update_block04 at (7, 5, 17).  Plant 1: _join is a no-op, the caller's stream never waits for the side stream -- the side stream
    held must differ.  Plant 2: _pre_pending is forgotten behind set_inp, update() never waits for _ev_pre -- the pre-activation stream held must differ."""
    case = EngineCase(model, "update_block04", 7, 5, 17, False)
    delay, want, _ = unheld(case.label, case.roles, case.run, case.prepare)
    set_inp = case.eng.set_inp

    def set_inp_and_forget(inp):
        set_inp(inp)
        case.eng._pre_pending = False

    for what, name, patch, role in (("1 (_join is a no-op)", "_join", lambda: None, "side:update_block04"),
                                    ("2 (_pre_pending forgotten)", "set_inp", set_inp_and_forget, "pre:update_block04")):
        with monkeypatch.context() as m:
            m.setattr(case.eng, name, patch)
            for held in (None, role):
                with case.alone(held) as roles:
                    got, _ = held_run(f"plant {what}", held, roles, delay, case.run, case.prepare)
                diff = R.differences(got, want)
                print(f"plant {what}, {held or 'nothing'} held: {len(diff)} differences, first {diff[:6]}")
        assert any(k in ("flow", "up", "net") for _, k, *_ in diff if isinstance(k, str)), (what, diff[:6])


def test_the_pipeline_tests_can_fail(model, timing):  # noqa: F811
    """Case (b).  Plant 3: pipeline.consumed is forgotten before every cascade call, so the next clip's 1/8 scale no longer waits for this clip's
    1/4-scale prologue -- with large held, that prologue reads the next clip's 1/8 state and the results must differ.  The held run needs a large
    stream whose delay holds back none of the streams the next clip's small scales run on (a process has fewer hardware queues than this case has
    streams, and at the streams' natural placement the plant stays hidden): CascadeCase.large_holds_nobody_else arranges that by measurement,
    before the plant runs, and the plant runs once."""
    case = the_cascade_case(model)
    want = check_cascade(case, "plain", None)
    case.prepare()
    diff = case.compare(case.run("plain", plant=True), want)
    print(f"\nplant 3 (consumed forgotten), nothing held: {len(diff)} differences {diff}")
    with case.large_holds_nobody_else() as replaced:
        print(f"streams replaced so that the 1/4 scale has a hardware queue of its own (name, pool streams tried): {replaced}")
        assert case.compare(held_run("b cascade plain, the 1/4 scale alone on its queue", "pipe.large", case.roles(False), case.reference("plain")[0],
                                     lambda: case.run("plain"), case.prepare)[0], want) == [], "without the plant"
        diff = case.compare(check_cascade(case, "plain", "pipe.large", plant=True), want)
    print(f"plant 3 (consumed forgotten), pipe.large held: {len(diff)} differences {diff}")
    assert diff and diff[0][0] in (0, 1), diff
