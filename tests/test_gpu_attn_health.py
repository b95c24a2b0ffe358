"""Fix-up accounting of the memory read-out: ppms_attn_redo_accumulate counts, on the device, the redo flags the rescale-free 64-query
kernel wrote (one per (clip, split, 256-query block) tile), ScaleEngine.enable_attn_health / attn_health / reset_attn_health keep them
over every call, and cascade / forward / forward_batch_test return them per scale.

Library-level shape: T = 3 clips, ksel = 3 picked frames, n = 320 pixels -- more than one split (3 with one frame per workgroup, 2 with
two), more than one 256-query block (g64 = 2) and a partly filled last block (64 of 256 queries)."""

import pytest
import torch

from ppmstereo_amd import weights as Wm
from ppmstereo_amd.weights import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, KSEL, N = 3, 3, 320
G64 = (N + 255) // 256
LOG2E = 1.4426950408889634
SCALE = 1.0
FRAMES = [pytest.param(1, id="one_frame_per_workgroup"), pytest.param(2, id="two_frames_per_workgroup")]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd import _lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    from ppmstereo_amd.ppmstereo import PPMStereoHotPath
    return PPMStereoHotPath().load_hot_path_weights(Wm.hot_path_weights()).to(DEV).eval()


def _operands(boost):
    """bf16-rounded Q (T,n,128), K' (T,ksel,n,128) and V (T,128,n) as fp32 CPU tensors.  Benign part: |q| ~ 11.3, keys 0.03 x normal, so
    a score is ~N(0, 0.34^2): inside +-2 everywhere (checked by the tests).  boost: list of (clip, query, slot, key): that query is made
    three times as long and that key receives 0.7 x the query's direction -- its score with the query rises to ~0.7 * 34 = 24 (34 log2
    units), with any other query to ~N(0, 0.7^2)."""
    q = hash_normal((T, N, 128), 1900)
    k = hash_normal((T, KSEL, N, 128), 1901) * 0.03
    v = hash_normal((T, 128, N), 1902)
    for clip, qi, slot, key in boost:
        d = q[clip, qi] / q[clip, qi].norm()
        q[clip, qi] *= 3.0
        k[clip, slot, key] += 0.7 * d
    return q.to(torch.bfloat16).float(), k.to(torch.bfloat16).float(), v.to(torch.bfloat16).float()


def _scores_log2(q, k):
    """fp64 scores in log2 units, [clip] -> (n, ksel * n), keys in slot order."""
    return [(q[c].double() @ k[c].reshape(-1, 128).double().t()) * (SCALE * LOG2E) for c in range(T)]


def _tile_excess(q, k, sps):
    """(T, nsp, g64) fp64: per tile, the largest excess (log2 units) of a score of the tile -- its 256 queries x the keys of its split's
    frames -- above that query's softmax reference in mem_attn64_kernel: the maximum over the first 32 keys of the split's FIRST frame
    (sub-tile 0 of the workgroup's first K tile)."""
    nsp = -(-KSEL // sps)
    out = torch.zeros(T, nsp, G64, dtype=torch.float64)
    for c, S in enumerate(_scores_log2(q, k)):
        for s in range(nsp):
            keys = S[:, s * sps * N:min((s + 1) * sps, KSEL) * N]
            ex = keys.max(1).values - keys[:, :32].max(1).values
            for b in range(G64):
                out[c, s, b] = ex[b * 256:(b + 1) * 256].max()
    return out


def _run(L, q, k, v, frames, p_format, calls=1, poison=True):
    """ppms_mem_attn + ppms_attn_redo_accumulate, `calls` times back to back on the current stream.  Returns (counters, raw output,
    redo flags as written: (T, nsp, g64, 2) int32, the int32 words behind them, workspace untouched by the accounting?)."""
    lib = L.load()
    qb, kb = q.to(torch.bfloat16).to(DEV), k.to(torch.bfloat16).to(DEV)
    vt = L.vt_image(v, p_format).to(DEV)
    sel = torch.tensor([[0, 1, 2, 0, 0]] * T, dtype=torch.int32, device=DEV)
    X = L.SPTensor(T * N, 256, DEV)
    beta = torch.tensor([1.0], device=DEV)
    raw = torch.zeros(T, N, 128, dtype=torch.bfloat16, device=DEV)
    nbytes = int(lib.ppms_mem_attn_workspace_bytes(T, KSEL, N))
    ws = torch.full((nbytes,), 0xFF if poison else 0, dtype=torch.uint8, device=DEV)
    counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    s = L.stream_ptr()
    for i in range(calls):
        L.check(lib.ppms_mem_attn(qb.data_ptr(), kb.data_ptr(), vt.data_ptr(), sel.data_ptr(), KSEL, SCALE, beta.data_ptr(), X.view(0, 128), X.view(128, 128),
                                  raw.data_ptr(), T, N, ws.data_ptr(), frames, p_format, s))
        before = ws.clone() if i + 1 == calls else None
        L.check(lib.ppms_attn_redo_accumulate(ws.data_ptr(), T, KSEL, N, frames, counters.data_ptr(), s))
    torch.cuda.synchronize()
    nsp = int(lib.ppms_mem_attn_splits(T, KSEL, N, frames))
    words = ws.view(torch.int32)[T * KSEL * N * 130:].cpu()
    used = T * nsp * G64 * 2
    return counters.tolist(), raw.float().cpu(), words[:used].reshape(T, nsp, G64, 2), words[used:], torch.equal(before, ws)


def _check_readout(got, q, k, v, p_format):
    """The per-element bound of tests/test_gpu_ops.py:_attn_check against the fp64 read-out x = softmax(Q K'^T scale) V on the bf16
    operands: |got - x| <= eps_P * (P |V|) (P~ rounded to p_format: 2^-11 fp16, 2^-8 bf16) + 2^-8 |x| (the bf16 result) + 1e-6, and a mean
    error inside half the mean bound."""
    eps_p = 2.0 ** -11 if p_format == 1 else 2.0 ** -8
    for c, S in enumerate(_scores_log2(q, k)):
        P = torch.softmax(S / LOG2E, dim=-1)
        V = torch.cat([v[f].t() for f in range(KSEL)]).double()            # sel = frames 0, 1, 2
        x = P @ V
        bound = eps_p * (P @ V.abs()) + 2.0 ** -8 * x.abs() + 1e-6
        err = (got[c].double() - x).abs()
        assert torch.isfinite(got[c]).all()
        worst = (err / bound).max().item()
        assert worst <= 1.0, f"clip {c}: element error {worst:.2f}x its bound"
        assert err.mean().item() <= 0.5 * bound.mean().item(), (err.mean().item(), bound.mean().item())


# ------------------------------------------------------------------------------------------------ 1: only written entries are read
@pytest.mark.parametrize("frames", FRAMES)
def test_only_the_written_flag_entries_are_counted(lib, frames):
    """Workspace pre-filled with 0xFF bytes, benign inputs (scores inside +-2): the call writes T * nsp * g64 flag pairs (nsp = 3 / 2),
    all zero; the pairs behind them -- sized for ksel splits -- keep the fill and must not be counted (counting T * ksel * g64 pairs, as
    the slice arithmetic of attn_redo_count does, reports them as flagged)."""
    L = lib
    q, k, v = _operands([])
    assert max(S.abs().max().item() for S in _scores_log2(q, k)) / LOG2E < 2.0
    nsp = {1: 3, 2: 2}[frames]
    assert L.load().ppms_mem_attn_splits(T, KSEL, N, frames) == nsp
    counters, raw, flags, tail, untouched = _run(L, q, k, v, frames, 1)
    print(f"frames_per_workgroup={frames}: counters {counters}")
    assert counters == [1, T * nsp * G64, 0]
    assert (flags == 0).all() and untouched, "the accounting kernel must leave the workspace as ppms_mem_attn wrote it"
    assert tail.numel() == T * (KSEL - nsp) * G64 * 2 and (tail == -1).all()      # never written: still the fill
    _check_readout(raw, q, k, v, 1)


# ------------------------------------------------------------------------------------------------ 2: flagged tiles are counted exactly
# (clip, split, 256-query block) tiles that receive a dominating key; splits 0 and 1 exist with one and with two frames per workgroup
CHOSEN = [(0, 0, 1), (1, 1, 0), (2, 1, 0), (2, 1, 1)]


def _boosted(sps):
    """One (clip, query, slot, key) per chosen tile: a query of the tile's block (block 1 holds queries 256 .. 319) and a key of the LAST
    frame of the tile's split, past that frame's first 32 keys -- so never among the 32 keys the reference maximum is taken over (the
    first 32 of the split's FIRST frame), whichever frame of the split it is."""
    out = []
    for i, (clip, split, blk) in enumerate(CHOSEN):
        slot = min((split + 1) * sps, KSEL) - 1
        out.append((clip, blk * 256 + 17 + 11 * i, slot, 100 + 53 * i))
    return out


@pytest.mark.parametrize("frames", FRAMES)
def test_flagged_tiles_are_counted_exactly(lib, frames):
    L = lib
    nsp = {1: 3, 2: 2}[frames]
    q, k, v = _operands(_boosted(frames))
    # the input property, in fp64: chosen tiles hold a score >= 24 log2 units above its query's reference (beyond fp16's 2^16, far inside
    # bf16's 2^60), every other tile stays below 8 -- no tile anywhere near either boundary
    ex = _tile_excess(q, k, frames)
    chosen = torch.zeros(T, nsp, G64, dtype=torch.bool)
    for c, s, b in CHOSEN:
        chosen[c, s, b] = True
    print(f"frames_per_workgroup={frames}: excess (log2) chosen tiles min {ex[chosen].min():.1f} max {ex[chosen].max():.1f}, other tiles max {ex[~chosen].max():.1f}")
    assert ex[chosen].min().item() >= 24.0 and ex[chosen].max().item() < 40.0 and ex[~chosen].max().item() < 8.0
    counters, raw, flags, _, untouched = _run(L, q, k, v, frames, 1)
    print(f"fp16 P~: counters {counters}")
    assert counters == [1, T * nsp * G64, len(CHOSEN)] and untouched
    assert torch.equal(flags[..., 0] != 0, chosen) and torch.equal(flags[..., 1] != 0, chosen)
    _check_readout(raw, q, k, v, 1)                                        # the flagged tiles took the fix-up pass: same bound
    counters, raw, flags, _, _ = _run(L, q, k, v, frames, 0)               # bf16 P~ carries 2^60: nothing to redo
    print(f"bf16 P~: counters {counters}")
    assert counters == [1, T * nsp * G64, 0] and (flags == 0).all()
    _check_readout(raw, q, k, v, 0)


# ------------------------------------------------------------------------------------------------ 3: accumulation over calls
def test_library_counters_accumulate_over_calls(lib):
    q, k, v = _operands(_boosted(1))
    one = _run(lib, q, k, v, 1, 1)[0]
    two = _run(lib, q, k, v, 1, 1, calls=2)[0]
    assert one == [1, T * 3 * G64, len(CHOSEN)] and two == [2 * x for x in one]


def test_engine_counters_accumulate_without_a_host_sync(model):
    """ScaleEngine at T = 3, 10 x 32 (n = 320, ksel = 3; the library's own choice is one frame per workgroup here: nsp = 3)."""
    from ppmstereo_amd import _lib as L
    dev = torch.device(DEV)
    eng = model.update_block04.engine(T, 10, 32, dev)
    for t_ in (eng.X, eng.Hb[0], eng.VAL):
        t_.set_f32(0.3 * hash_normal((t_.pixels, t_.channels), 1903).to(dev))
    eng.QB.copy_(hash_normal((T, N, 128), 1904).to(torch.bfloat16))
    eng.SEL[:, :3] = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    eng.SHAT.fill_(1.0)
    nsp = L.load().ppms_mem_attn_splits(T, eng.ksel, eng.n, 0)
    assert eng.n == N and eng.ksel == KSEL and nsp == 3
    with torch.cuda.device(dev):
        assert eng.attn_health() == {"calls": 0, "tiles": 0, "flagged": 0}          # never enabled: nothing counted, nothing allocated
        eng.attend()
        assert eng.attn_health() == {"calls": 0, "tiles": 0, "flagged": 0}
        eng.ATT_WS.fill_(0xFF)
        eng.enable_attn_health()
        eng.reset_attn_health()
        eng.attend()
        one = eng.attn_health()
        assert one["calls"] == 1 and one["tiles"] == T * nsp * G64 and 0 <= one["flagged"] <= one["tiles"]
        eng.reset_attn_health()
        eng.attend()
        eng.attend()                                                              # (nothing between the two calls touches the host)
        two = eng.attn_health()
        assert two == {k_: 2 * v_ for k_, v_ in one.items()}
        eng.reset_attn_health()
        eng.attend()
        assert eng.attn_health() == one
        eng.enable_attn_health(False)                                             # off again: the counters stay where they are
        eng.attend()
        assert eng.attn_health() == one


# ------------------------------------------------------------------------------------------------ 4: the results are untouched
def _cascade_both_ways(model, feats, iters, t):
    feats = {k_: v_.to(DEV) for k_, v_ in feats.items()}
    p0, u0, p1, u1 = [], [], [], []
    model.cascade(dict(feats), iters, t, p0, u0)
    diag = {}
    model.cascade(dict(feats), iters, t, p1, u1, diagnostics=diag)
    torch.cuda.synchronize()
    assert len(p0) == len(p1) == 2 * (iters // 2) + iters
    for a, b in zip(p0 + u0, p1 + u1):
        assert torch.equal(a, b), "accounting changed a prediction / uncertainty"
    return diag


def _expected(lib, t, n, calls):
    nsp = lib.load().ppms_mem_attn_splits(t, min(5, t), n, 0)
    return {"calls": calls if nsp else 0, "tiles": calls * t * nsp * ((n + 255) // 256), "flagged": None}


def test_cascade_diagnostics_leave_the_results_untouched(lib, model):
    """The geometry of the cascade_it10 fixture (T = 5, 64 x 256: n = 64, 256, 1024; 5 / 5 / 10 iterations), with and without
    diagnostics: every prediction and uncertainty bit-identical, per scale calls == iterations and tiles == calls * T * nsp * g64."""
    from ppmstereo_amd.synth import synth_cascade_feats
    t, H, W, iters = 5, 64, 256, 10
    diag = _cascade_both_ways(model, synth_cascade_feats(t, H, W), iters, t)
    print(f"attn_redo: {diag['attn_redo']}")
    assert set(diag) == {"attn_redo"} and list(diag["attn_redo"]) == ["1/16", "1/8", "1/4"]
    for s_, n_it in ((16, iters // 2), (8, iters // 2), (4, iters)):
        got, want = diag["attn_redo"][f"1/{s_}"], _expected(lib, t, (H // s_) * (W // s_), n_it)
        assert got["calls"] == want["calls"] == n_it and got["tiles"] == want["tiles"] > 0 and 0 <= got["flagged"] <= got["tiles"]
    # a second call with the same dict adds onto the entries already there
    first = {k_: dict(v_) for k_, v_ in diag["attn_redo"].items()}
    model.cascade({k_: v_.to(DEV) for k_, v_ in synth_cascade_feats(t, H, W).items()}, iters, t, test_mode=True, diagnostics=diag)
    assert diag["attn_redo"] == {k_: {c: 2 * x for c, x in v_.items()} for k_, v_ in first.items()}
    # the engines are left as they were: accounting off
    assert not model.update_block04.engine(t, H // 4, W // 4, torch.device(DEV))._health_on


def test_cascade_diagnostics_are_zero_where_the_32_query_kernel_runs(lib, model):
    """96 x 256: the 1/16 scale has n = 6 x 16 = 96 pixels, no multiple of 64 -- the 32-query kernel serves it, no flags exist: all zeros."""
    from ppmstereo_amd.synth import synth_cascade_feats
    t, H, W, iters = 2, 96, 256, 2
    diag = _cascade_both_ways(model, synth_cascade_feats(t, H, W), iters, t)
    print(f"attn_redo: {diag['attn_redo']}")
    assert diag["attn_redo"]["1/16"] == {"calls": 0, "tiles": 0, "flagged": 0}
    for s_, n_it in ((8, 1), (4, 2)):
        got, want = diag["attn_redo"][f"1/{s_}"], _expected(lib, t, (H // s_) * (W // s_), n_it)
        assert got["calls"] == n_it and got["tiles"] == want["tiles"] > 0


# ------------------------------------------------------------------------------------------------ 5: forward_batch_test
def test_forward_batch_test_reports_the_sum_over_windows(lib):
    """Stub encoders (tests/stub_encoders.py), 5 frames of 64 x 256, kernel_size 4: two windows, [0, 4) and [2, 5), pipelined -- the
    counters are read in ClipPipeline.wait() -- against the same two windows run one by one through forward()."""
    from ppmstereo_amd.ppmstereo import PPMStereo, window_plan
    from stub_encoders import StubCNet, StubFNet, frame_video
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(Wm.hot_path_weights()).to(DEV).eval()
    video = frame_video(5, 64, 256)
    plan = window_plan(5, 4)
    assert [(a, b) for a, b, _, _ in plan] == [(0, 4), (2, 5)]
    plain = m.forward_batch_test({"stereo_video": video}, kernel_size=4, iters=2)
    assert set(plain) == {"disparity", "uncertainties"}
    out = m.forward_batch_test({"stereo_video": video}, kernel_size=4, iters=2, diagnostics=True)
    assert set(out) == {"disparity", "uncertainties", "attn_redo"}
    assert torch.equal(out["disparity"], plain["disparity"]) and torch.equal(out["uncertainties"], plain["uncertainties"])
    total = {}
    for start, stop, _, _ in plan:
        win = video[start:stop].to(DEV)
        d = {}
        m.forward(win[None, :, 0], win[None, :, 1], iters=2, test_mode=True, diagnostics=d)
        t = stop - start
        for s_, n_it in ((16, 1), (8, 1), (4, 2)):
            want = _expected(lib, t, (64 // s_) * (256 // s_), n_it)
            assert d["attn_redo"][f"1/{s_}"]["calls"] == n_it and d["attn_redo"][f"1/{s_}"]["tiles"] == want["tiles"]
            acc = total.setdefault(f"1/{s_}", {"calls": 0, "tiles": 0, "flagged": 0})
            for c, x in d["attn_redo"][f"1/{s_}"].items():
                acc[c] += x
    print(f"attn_redo over two windows: {out['attn_redo']}")
    assert out["attn_redo"] == total and total["1/4"]["calls"] == 4
