"""bench.py's two modes on the tiny UNet (-m gpu): a plain run reports the headline figure only; --full adds power / clock,
value_dedup and the roofline after the same timed steps (cpu_baseline is left out here: it is minutes of host time)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--tiny", "--images-per-step", "2", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_reports_the_headline_only(dev):
    d = _bench()
    assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["value_dedup"] is None and d["dedup"] is None
    for k in ("power", "roofline", "cpu_baseline", "cpu_baseline_config0"):
        assert k not in d, k


def test_full_run_adds_dedup_power_and_roofline(dev):
    d = _bench("--full", "--no-cpu-baseline")
    assert all(k in d for k in HEADLINE) and d["value"] > 0
    assert d["dedup"]["latents_bitwise_equal_to_full_run"] is True and d["value_dedup"] > 0
    assert "power" in d
    r = d["roofline"]
    assert r["achieved"] > 0 and r["launches_per_step"] > 0 and "attention" in r["families"]
    assert "cpu_baseline" not in d
