"""bench.py's two kinds of run on a small configuration: a plain run prints the headline line (and --dump-outputs) and
nothing else; --full adds the profiled pass, fwd_only and the CPU baseline after the timed region."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--batch", "8", "--size", "64", "--steps", "2", "--warmup", "2"]
FULL_ONLY = ("profiled", "kernel_classes", "roofline", "fwd_only", "secondary", "cpu_baseline")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only(tmp_path):
    r = _bench("--dump-outputs", str(tmp_path / "out"))
    assert r["metric"] == "instance-pairs/sec (fwd+bwd)" and r["unit"] == "pairs/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 2 and r["value"] > 0 and r["ms_per_step"] > 0
    assert abs(r["value"] - 8 * 1e3 / r["ms_per_step"]) < 1e-6 * r["value"]
    assert not [k for k in FULL_ONLY if k in r], r.keys()
    assert "profiled pass" not in r["config"]["timed_region"]
    assert "loss" in r["dump_outputs"]["arrays"] and os.path.exists(tmp_path / "out" / "loss.npy")


def test_full_run_adds_the_secondary_measurements():
    r = _bench("--full")
    assert r["value"] > 0 and r["ms_per_step"] > 0
    for k in ("profiled", "kernel_classes", "roofline", "fwd_only", "cpu_baseline"):
        assert k in r, k
    assert "secondary" not in r                     # the secondary legs belong to the headline configuration only
    assert "failed" not in r["fwd_only"] and r["cpu_baseline"]["value"] > 0
    assert "profiled pass" in r["config"]["timed_region"]
