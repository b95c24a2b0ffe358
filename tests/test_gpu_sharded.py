"""GPU: the frame-sharded engine (SURVEY.md section 8e level 2, BASELINE configs 4-5) on the real kernels.  One GPU box has one
GPU, so two ranks share it and talk over gloo (dist.FrameShard stages device tensors through the host in that case; on a
multi-GPU node the same calls go through RCCL).  Each rank runs its block of frames of a T = 8 window through the whole 3-scale
cascade and compares with the unsharded cascade run in the same process -- and a T = 10 window over two ranks at the per-GPU geometry of
BASELINE configs 4 and 5, where the 1/4 scale runs the large-map kernels with temporal halos."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, c3d, T=8, H=64, W=256, census=False):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ppmstereo_amd import dist as D
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereoHotPath
    from ppmstereo_amd.synth import synth_cascade_feats
    D.init_from_env("gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    iters = 4
    model = PPMStereoHotPath(use_convex_3d=c3d).load_hot_path_weights(Wm.hot_path_weights(use_convex_3d=c3d)).to(dev).eval()
    feats = synth_cascade_feats(T, H, W, seed=5)
    shard = D.FrameShard(rank, world, T)
    local = {k: v[shard.lo:shard.hi].to(dev) for k, v in feats.items()}
    p1, u1 = [], []
    d_sh, c_sh = model.cascade(local, iters, T, p1, u1, shard=shard)
    torch.cuda.synchronize()
    halo_forms = None
    if census:                      # the launches of the 1/4-scale engine that read halo slabs, by launch form (test_gpu_ops.conv_form)
        from ppmstereo_amd.engine import ConvOp
        from test_gpu_ops import conv_form
        eng = next(e for e in model.update_block04._engines.values() if e.halo > 0)
        assert (eng.T, eng.h, eng.w) == (shard.f, H // 4, W // 4)
        halo_forms = {}
        for name, op in eng.op.items():
            if isinstance(op, ConvOp) and op.desc.t_halo > 0:
                assert op.desc.t_halo == eng.halo, name
                halo_forms.setdefault(conv_form(op), []).append(name)
    D.barrier()
    d_full, c_full = model.cascade({k: v.to(dev) for k, v in feats.items()}, iters, T)
    torch.cuda.synchronize()
    sl = slice(shard.lo, shard.hi)
    res = dict(disp=(d_sh - d_full[sl]).abs().max().item(), unc=(c_sh - c_full[sl]).abs().max().item(), npred=len(p1),
               finite=bool(torch.isfinite(d_sh).all()), scale=d_full.abs().max().item(), census=halo_forms)
    torch.save(res, out + f".{rank}")
    D.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world,c3d", [(2, False), (2, True), (4, False)])
def test_sharded_cascade_equals_unsharded_on_the_gpu(tmp_path, world, c3d):
    """All three scales (update_block16 with its temporal attention gather, 08, 04), 2 / 2 / 4 iterations, K / V / confidence
    all-gathers and every temporal halo, against the same cascade on one rank.  The kernels compute every pixel from the same
    operands whichever rank holds it (zero halos stand for the window's zero padding); what differs is the launch plan -- a rank
    with half the frames has half the tiles, so the K-sliced convolutions of the small scales split their sums differently -- i.e.
    fp32 summation order, which the loop amplifies like any other rounding (measured 2.5e-4 px after 8 predictions).  A missing
    exchange shows as 0.1-1 px (tests/test_dist_gloo.py has the fault-injection twin).
    world = 4: two frames per rank (= the halo depth), interior ranks with two neighbours, three peers in the direct all-gather."""
    out = str(tmp_path / "sh.pt")
    mp.spawn(_worker, args=(world, _free_port(), out, c3d), nprocs=world, join=True)
    for r in range(world):
        res = torch.load(out + f".{r}")
        assert res["finite"] and res["npred"] == 8
        assert res["disp"] <= 5e-5 * max(1.0, res["scale"]), res
        assert res["unc"] <= 2e-4, res


@pytest.mark.parametrize("H,W,c3d", [pytest.param(320, 512, False, id="config4"), pytest.param(320, 512, True, id="config4_c3d"),
                                       pytest.param(736, 1280, False, id="config5")])
def test_sharded_cascade_at_a_baseline_rank_geometry(tmp_path, H, W, c3d):
    """BASELINE configs 4 / 5 per GPU: 5 frames of a T = 10 window on each of two ranks -- at 320 x 512 a 5 x 80 x 128 map at the 1/4 scale (config 4),
    at 736 x 1280 a 5 x 184 x 320 one (config 5) -- large enough for the library to rate conv_gemm6 there, so the GRU's pass T (5,1,1) and the 3x3x3
    heads run on the large-map kernels with t_halo > 0 (the T = 8, 64 x 256 test above runs only the small-map kernels).  Each rank takes a census of its 1/4-scale engine's halo'd launches by
    form: it must hold conv_gemm6 launches with kt = 5 and kt = 3, and every form must be one that test_gpu_ops.test_conv_temporal_halo_vs_fp64
    checks with a halo (HALO_COVERED_FORMS).  Then the same bounds as above against the unsharded cascade of the same process.
    (What the census finds at both sizes: conv_gemm6 for the 256-row (5,1,1) convs pre_zr3 / zr3 / zr3_x and the 3x3x3 fh1 -- and m1 with
    use_convex_3d --, conv_gemm2 for the 128-row (5,1,1) convs pre_q3 / q3 / q3_x: conv_gemm6's STREAM form is packed for > 128 rows only.)"""
    from test_gpu_ops import HALO_COVERED_FORMS
    world = 2
    out = str(tmp_path / "shb.pt")
    mp.spawn(_worker, args=(world, _free_port(), out, c3d, 10, H, W, True), nprocs=world, join=True)
    for r in range(world):
        res = torch.load(out + f".{r}")
        census = res["census"]
        print(f"[halo census] {H}x{W} rank {r} c3d={c3d}: " + "; ".join(f"{k}: {' '.join(v)}" for k, v in sorted(census.items())))
        print(f"[sharded T=10 {H}x{W}] rank {r} c3d={c3d}: disp {res['disp']:.3e} (bound {5e-5 * max(1.0, res['scale']):.3e}), "
              f"unc {res['unc']:.3e} (bound 2e-4)")
        assert any(k[0] == 8 and k[1] == 5 for k in census) and any(k[0] == 8 and k[1] == 3 for k in census), census
        missing = {k: v for k, v in census.items() if k not in HALO_COVERED_FORMS}
        assert not missing, f"halo'd launch forms without a kernel-level halo test: {missing}"
        assert res["finite"] and res["npred"] == 8
        assert res["disp"] <= 5e-5 * max(1.0, res["scale"]), res
        assert res["unc"] <= 2e-4, res


def _window_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ppmstereo_amd import dist as D
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo
    from stub_encoders import StubCNet, StubFNet, frame_video
    D.init_from_env("gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    m = PPMStereo.shipped(fnet=StubFNet(), cnet=StubCNet(), sst=None).load_hot_path_weights(Wm.hot_path_weights()).to(dev).eval()
    video = frame_video(45, 60, 250)                        # kernel_size 20: windows [0,20) [10,30) [20,40) [30,45)
    sharded = m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=2, shard_ranks=True)
    torch.cuda.synchronize()
    D.barrier()
    res = dict(shape=tuple(sharded["disparity"].shape))
    if rank == 0:
        full = m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=2)
        res.update(equal=bool(torch.equal(full["disparity"], sharded["disparity"]) and torch.equal(full["uncertainties"], sharded["uncertainties"])),
                   nonzero=bool((sharded["disparity"].abs().amax((1, 2, 3)) > 0).all()))
    torch.save(res, out + f".{rank}")
    D.barrier()
    torch.distributed.destroy_process_group()


def test_window_sharded_forward_batch_test_on_the_gpu(tmp_path):
    """SURVEY 8e level 1 with a driver on the GPU: forward_batch_test(shard_ranks=True) deals the sliding windows of a 45-frame video
    round-robin over two ranks (independent units, no data-path collective), gathers the kept frames once at the end
    (dist.gather_kept_frames) and must return, on every rank, exactly the single-process result (same kernels per window)."""
    out = str(tmp_path / "win.pt")
    mp.spawn(_window_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert r0["shape"] == r1["shape"] == (45, 1, 60, 250)
    assert r0["equal"] and r0["nonzero"], r0


def _bench_line(argv, timeout=560):
    """python bench.py <argv> with no launcher around it (bench.launch_ranks starts the ranks), gloo between the ranks: both share this box's
    one GPU, device tensors are staged through the host by dist.FrameShard -- a rehearsal of the N > 1 bench paths with the REAL kernels, never
    a measurement (on a multi-GPU node the same command line runs over RCCL, one rank per GPU)."""
    import json
    import subprocess
    env = dict(os.environ, PPMS_DIST_BACKEND="gloo", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, cwd=ROOT, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("T,scaling", [(5, "weak"), (8, "strong")])
def test_bench_gpus_2_runs_end_to_end_on_one_gpu_over_gloo(T, scaling):
    """`python bench.py --gpus 2`: two ranks launched by bench.py itself; T = 5 -> clip replicas (what the driver's scaling run does at
    config 2), T = 8 -> the window's frames sharded 4 + 4 with every exchange of dist.FrameShard inside the timed steps."""
    out = _bench_line(["--gpus", "2", "--T", str(T), "--H", "64", "--W", "256", "--iters", "4", "--steps", "2", "--warmup", "1",
                       "--full", "--no-cpu-baseline", "--no-encoders", "--sharded-T", "8", "--sharded-iters", "4", "--sharded-steps", "1"])
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["value"] > 0 and out["steps"] == 2
    px = T * 64 * 256
    want = (1 if scaling == "strong" else 2) * 2 * px / (out["ms_per_step"] * 2e-3)
    assert abs(out["value"] - want) <= 1e-3 * want          # value = whole-job pixels over the max-over-ranks time of exactly K steps
    assert ("sharded" in out["config"]["parallelism"]) == (scaling == "strong")
    if scaling == "weak":                # replicas as the measurement: ONE extra frame-sharded window (here T = 8, 4 + 4 frames) on the same ranks, checked
        sh, chk = out["sharded"], out["sharded_check"]          # against the unsharded result on rank 0 before it is timed
        assert sh["T"] == 8 and sh["frames_per_gpu"] == 4 and sh["ms_per_window"] > 0 and sh["scaling"] == "strong" and "rehearsal" in sh["note"]
        assert chk["passed"] and chk["max_abs_disparity_diff_px"] <= chk["tolerance_px"]
    else:
        assert out["sharded"] is None
