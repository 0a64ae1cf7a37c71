"""bench.py end to end on the GPU: the instrumented steps of a `--full` run wrap every spx.ops entry point, so a new keyword
argument in ops that the wrappers do not pass through breaks that run (it did once, round 3); a plain run prints the headline
line alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_with_roofline_and_kernels(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    dump = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--full",
                        "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(dump)], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-500:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("point-cloud frames/sec") and d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0
    assert d["ms_per_step"] > 0
    # --dump-outputs: the last timed training step's loss, gradients and updated parameters, float32 / float64, <= 64 MB
    files = {f.name[:-4]: f for f in dump.iterdir()}
    assert sum(f.stat().st_size for f in files.values()) <= 64_000_000
    assert "loss" in files and any(k.startswith("grad.backbone_3d.") for k in files) and any(k.startswith("param.") for k in files)
    for k, f in files.items():
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), k
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0.0 < r["frac"] < 1.0 and r["achieved"] > 0 and r["peak"] > 0
    assert r["traffic"] is None or r["traffic"] > 0
    k = d["kernels"]
    for fam in ("subm_rulebook", "conv_rulebook", "conv_gemm[mfma 64x64 ring]", "conv_ring_plan", "densify(+memset)"):
        assert fam in k and k[fam]["ms_per_step"] > 0 and k[fam]["bound"] in ("hbm", "mfma"), fam


def test_bench_outputs_repeat_bit_for_bit(tmp_path):
    """Two runs of the same training benchmark compute the same last step: same seeded inputs, and every reduction of the
    step in a fixed order (spx kernels; the BEV tail's stock-conv weight gradients via model_utils/det_wgrad.py — MIOpen's
    backward-weights reduces in a run-dependent order, and AdamW's first steps amplify its last-bit differences).  Ten
    steps, so a difference in any step reaches the dumped loss, gradients and parameters.  Both are plain runs (no --full):
    their line carries the headline and none of the legs that take runs of their own."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    dumps = []
    for run in ("a", "b"):
        dumps.append(tmp_path / run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "4",
                            "--dump-outputs", str(dumps[-1])], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-500:]
        d = json.loads(lines[0])
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 6 and d["warmup"] == 4
        assert not {"roofline", "kernels", "extras", "cpu_baseline"} & set(d), sorted(d)
    names = sorted(f.name for f in dumps[0].iterdir())
    assert names == sorted(f.name for f in dumps[1].iterdir()) and len(names) > 100
    differ = [n for n in names if not np.array_equal(np.load(dumps[0] / n), np.load(dumps[1] / n))]
    assert differ == [], differ[:10]
