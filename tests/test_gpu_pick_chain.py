"""GPU: the merged pick + key modulation launch of the memory read-out chain against the library's own unmerged entries, bit for bit.

  * ppms_pick_prep_k (QAM pick inside the key modulation launch) vs ppms_qam_select + ppms_attn_prep_k;
  * ScaleEngine.iterate() (which uses it) vs the stages called one by one (pick() + attend(): the unmerged pick).

(The other merge tried with it -- fix-up pass + merge of the attention partials as one launch -- did not win on the clip and is not in the
library: docs/LOG_r08.md; its test left with it.)

Every comparison is on raw bits (integer views: NaNs -- T == 1 -- compare by their bit patterns too)."""
import pytest
import torch

from ppmstereo_amd import _lib as L
from ppmstereo_amd.synth import synth_scale_inputs
from ppmstereo_amd.weights import hash_normal
from test_gpu_block import DEV, W, model  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ pick + key modulation
@pytest.mark.parametrize("T,n,ld", [(5, 64, 256), (2, 100, 128), (7, 192, 256), (1, 64, 128)])
def test_pick_prep_k_equals_select_then_prep(T, n, ld):
    """Six consecutive picks with the evolving usage counter: SEL, SHAT, SCORE, the counter and K' after every one.  Reference: ppms_qam_select
    (counter in place) + ppms_attn_prep_k; under test: ppms_pick_prep_k with the ping-pong counter pair.  K' buffers are pre-filled with a
    pattern, slots 'behind' ksel do not exist in the [clip][ksel][n][128] layout, so the guard rows behind the last clip stand for everything
    neither path may touch.  T = 7: ksel = 5 < T -- the confidences are arranged so that one frame is picked by nobody and another by all
    seven clips in some iteration (the merged kernel's per-frame lists have 0 .. T entries).  T = 1: the score is NaN."""
    from ppmstereo_amd.engine import temporal_pe
    lib, s = L.load(), L.stream_ptr()
    ksel, nblk, guard = min(5, T), (n + 255) // 256, 4 * 128
    sim = torch.tanh(hash_normal((T, T), 1300 + T)).to(DEV)
    if T == 1:
        sim.fill_(float("nan"))
    keyfull = hash_normal((T * n, ld), 1310 + T).to(DEV)
    off = ld - 128                                                    # the engine's layout: keys in the upper half of a [q | k] row
    key_ptr = keyfull.data_ptr() + off * 4
    pe = temporal_pe(T, 128).to(DEV)
    strive_ref = torch.ones(T, T, device=DEV)
    strive = [torch.ones(T, T, device=DEV), torch.full((T, T), -7.0, device=DEV)]      # [current, next]
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=DEV)
    sel_r, sel_m = z(T, 5, dt=torch.int32), z(T, 5, dt=torch.int32)
    shat_r, shat_m, score_r, score_m = z(T, 5), z(T, 5), z(T, T), z(T, T)
    kb_r = torch.empty(T * ksel * n * 128 + guard, dtype=torch.bfloat16, device=DEV)
    kb_m = torch.empty_like(kb_r)
    counts = []
    for it in range(6):
        part = (0.5 + 0.5 * torch.rand(T, nblk, generator=torch.Generator().manual_seed(1320 + 10 * T + it))) * min(n, 256)
        if T == 7 and it == 2:
            part[3] = -40.0 * n                                       # frame 3: confidence far below every other score -> nobody picks it
            part[5] = 40.0 * n                                        # frame 5: every clip picks it
        part = part.to(DEV)
        for kb in (kb_r, kb_m):
            bits(kb).fill_(0x7B7B)
        for t in (sel_r, sel_m):
            t.fill_(-1)
        for t in (shat_r, shat_m, score_r, score_m):
            t.fill_(-3.0)
        L.check(lib.ppms_qam_select(sim.data_ptr(), strive_ref.data_ptr(), part.data_ptr(), nblk, n, sel_r.data_ptr(), shat_r.data_ptr(),
                                    score_r.data_ptr(), T, s))
        L.check(lib.ppms_attn_prep_k(key_ptr, ld, pe.data_ptr(), sel_r.data_ptr(), shat_r.data_ptr(), kb_r.data_ptr(), T, ksel, n, s))
        L.check(lib.ppms_pick_prep_k(sim.data_ptr(), strive[0].data_ptr(), strive[1].data_ptr(), part.data_ptr(), nblk, n, sel_m.data_ptr(),
                                     shat_m.data_ptr(), score_m.data_ptr(), key_ptr, ld, pe.data_ptr(), kb_m.data_ptr(), T, n, s))
        strive.reverse()
        torch.cuda.synchronize()
        assert same(sel_m, sel_r), (it, sel_m.tolist(), sel_r.tolist())
        assert same(shat_m, shat_r), it
        assert same(score_m, score_r), it
        assert same(strive[0], strive_ref), (it, strive[0].tolist(), strive_ref.tolist())
        assert same(kb_m, kb_r), it
        assert (bits(kb_r[-guard:]) == 0x7B7B).all() and (bits(kb_m[-guard:]) == 0x7B7B).all(), "a write behind the last [clip][slot]"
        assert (bits(kb_r[:-guard]) != 0x7B7B).any()
        counts.append(torch.bincount(sel_r[:, :ksel].flatten().cpu(), minlength=T))
    counts = torch.stack(counts)
    assert int(strive_ref.sum().item()) == T * T + 6 * T * ksel        # the counter really evolved
    if T == 7:
        assert (counts < T).any(), "ksel < T: some frame must be unpicked by some clip"
        assert int(counts[2, 3]) == 0 and int(counts[2, 5]) == T, counts.tolist()       # list lengths 0 and T both occurred


# ------------------------------------------------------------------------------------------------ engine
# (2, 5, 17), n = 85: the generic attention path (n % 64 != 0).  The lookup stage needs a 4-level correlation pyramid, i.e. w >= 16 (the
# library refuses narrower maps, as the reference fails on them), so a 5 x 9 map (n = 45) cannot run an iteration: the smallest odd-sized map
# with a 5-row height that can is used instead.
@pytest.mark.parametrize("T,h,w", [(3, 16, 32), (2, 5, 17)])
def test_iterate_equals_stages_called_separately(model, T, h, w):  # noqa: F811
    """Two engines of the 1/4-scale block, same weights and inputs, three iterations: iterate() (merged pick + key modulation) against lookup,
    motion_and_value, uncertainty, pick, attend, update called one by one (ppms_qam_select, then ppms_attn_prep_k)."""
    from ppmstereo_amd.corr import CorrBlock1D
    dev = torch.device(DEV)
    d = {k: (None if v is None else v.to(DEV)) for k, v in synth_scale_inputs(T, h, w, seed=131, with_mhs=True, frame_contrast=1.0).items()}
    blk = model.update_block04
    engs = [blk.engine(T, h, w, dev, slot=0), blk.engine(T, h, w, dev, slot=1)]
    assert engs[0] is not engs[1] and engs[0].shard is None
    assert (engs[0].n % 64 == 0) == ((T, h, w) == (3, 16, 32))
    out = []
    with torch.cuda.device(dev):
        for eng in engs:
            eng.set_inp(d["inp"]), eng.set_net(d["net"]), eng.set_flow(d["flow"]), eng.set_mhs(d["mhs"])
            eng.begin(CorrBlock1D(d["fmap1"], d["fmap2"]).levels, model.att[2].packed(dev))
        for it in range(3):
            up0 = engs[0].iterate()
            e = engs[1]
            e.lookup(), e.motion_and_value(), e.uncertainty(), e.pick(), e.attend(), e.update()
            up1 = e.upsample()
            torch.cuda.synchronize()
            state = [[x.get_flow(), x.get_net(), x.get_mhs(), x.SEL.clone(), x.SHAT.clone(), x.STRIVE.clone(), x.SCORE.clone(), x.KB.clone()] for x in engs]
            for name, a, b in zip(("flow", "net", "mhs", "SEL", "SHAT", "STRIVE", "SCORE", "K'"), *state):
                assert same(a, b), (it, name)
            assert same(up0, up1), it
            out.append(state[0][0])
    assert int(engs[0].STRIVE.sum().item()) == T * T + 3 * T * engs[0].ksel
    assert torch.isfinite(out[-1]).all() and not same(out[-1], out[0])
