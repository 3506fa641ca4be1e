"""bench.py as the headline is taken: a plain run prints the headline and nothing that needs checks or runs of its own;
--full adds them and times the same steps on the same inputs.  Needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(tmp_path, name, *args):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)] + list(args),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


def test_plain_and_full_bench_lines(tmp_path):
    plain, plain_dir = _bench(tmp_path, "plain")
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["metric"] == "frame-pairs/s + achieved HBM GB/s, 720x480 bs=16 sw=16 exhaustive"
    assert plain["config"]["pairs_per_step_per_gpu"] == 2048 and "outputs_dumped" in plain
    for k in ("parity", "roofline", "secondary", "content_sweep", "pcie_inclusive", "cpu_baseline", "cpu_baseline_c"):
        assert k not in plain, k

    full, full_dir = _bench(tmp_path, "full", "--full", "--no-secondary", "--no-cpu-baseline", "--no-content-sweep", "--no-pcie")
    assert all(k in full for k in HEADLINE) and full["metric"] == plain["metric"]
    assert full["parity"]["ok"] and full["parity"]["pairs_checked"] >= 3 and full["parity"]["pair0_equals_reference_golden"]
    assert full["roofline"]["kernel_ms_per_launch"] > 0 and "secondary" not in full
    names = sorted(os.listdir(plain_dir))
    assert names == sorted(os.listdir(full_dir)) == ["mv.npy"]
    assert np.array_equal(np.load(plain_dir / "mv.npy"), np.load(full_dir / "mv.npy"))
