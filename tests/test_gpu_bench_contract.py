"""GPU: `python bench.py --full` at N = 1 on BASELINE config 2 prints ONE JSON line that carries the contract's fields: the metric and its
configuration, `roofline` (dominant kernel: bound, achieved, peak, unit, frac, traffic), `cpu_baseline` (value, unit, cores, kind, sample), and the
library that ran.  The plain command (no --full) prints the headline fields only and, with --dump-outputs, writes the last timed step's outputs.
Short runs (2-3 steps): the numbers are not asserted beyond consistency, the shape of the line is."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(*argv):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PPMS_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True, cwd=ROOT, env=env, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_n1_line_has_the_contract_fields():
    out = _bench_line("--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-encoders")
    assert out["metric"] == "disparity-px/s" and out["unit"] == "disparity-px/s" and out["higher_is_better"] is True
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert out["data"] == "synthetic" and out["dtype"] == "bf16"
    cfg = out["config"]
    assert "BASELINE config 2" in cfg["workload"] and (cfg["T"], cfg["H"], cfg["W"], cfg["iters"]) == (5, 320, 512, 10) and "model" not in cfg
    px = 5 * 320 * 512
    assert abs(out["value"] - px / (out["ms_per_step"] * 1e-3)) <= 2e-3 * out["value"]          # value = pixels of K steps / their wall time
    for key in ("roofline", "roofline_2", "roofline_3", "roofline_hbm"):
        rf = out[key]
        assert rf["bound"] in ("mfma", "hbm") and rf["unit"] in ("TFLOP/s", "GB/s") and rf["peak"] > 0 and "traffic" in rf
        assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 2e-3 and 0 < rf["frac"] < 1
    assert "conv6_kernel" in out["roofline"]["kernel"] or "memory attention" in out["roofline"]["kernel"]
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "disparity-px/s" and cb["value"] > 0 and 1 <= cb["cores"] <= 16 and "iterations" in cb["sample"]
    assert out["library"] == "ppmstereo_amd/libppms.so" and out["build_mode"] in ("reused", "compiled") and out["library_stamp_matches_sources"] is True
    assert out["sharded"] is None and out["sharded_check"] is None


def test_bench_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    """The plain command: the headline fields of K = 3 timed steps, nothing measured beside them, and --dump-outputs: what the timed path returned
    in its last step -- disparity and uncertainty, (T, 1, H, W) float32 each, finite, 6.6 MB together (under the 64 MB cap: not sampled)."""
    import numpy as np
    d = tmp_path / "outputs"
    out = _bench_line("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    assert out["metric"] == "disparity-px/s" and out["unit"] == "disparity-px/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False and out["ms_per_step"] > 0
    px = 5 * 320 * 512
    assert abs(out["value"] - px / (out["ms_per_step"] * 1e-3)) <= 2e-3 * out["value"]
    for key in ("roofline", "roofline_2", "roofline_3", "roofline_hbm", "cpu_baseline", "latency_ms_per_clip", "ms_per_step_all_predictions",
                "whole_call_ms", "encoders", "sharded"):
        assert key not in out, key
    assert sorted(os.listdir(d)) == ["disparity.npy", "uncertainty.npy"]
    assert out["outputs"] == {n: dict(shape=[5, 1, 320, 512], stride=1) for n in ("disparity", "uncertainty")}
    total = 0
    for name in ("disparity", "uncertainty"):
        a = np.load(d / (name + ".npy"))
        total += (d / (name + ".npy")).stat().st_size
        assert a.dtype == np.float32 and a.shape == (5, 1, 320, 512) and np.isfinite(a).all(), name
    assert np.load(d / "disparity.npy").std() > 0
    assert total <= 64 * 2 ** 20
