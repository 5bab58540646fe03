"""bench.py's two kinds of run on the GPU: a plain run prints the headline line only; --full adds the extra legs after it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
LEGS = ("roofline", "cpu_baseline", "other_configs")


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--ddim-steps", "3"] + args,
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only():
    rec = _bench([])
    assert all(k in rec for k in HEADLINE), sorted(rec)
    assert rec["metric"] == "512px 50-step char images/sec (node), CMIGBench 4-turn story"
    assert rec["unit"] == "char_images/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 1 and rec["warmup"] == 0
    assert not any(k in rec for k in LEGS), sorted(rec)


def test_full_run_adds_the_roofline_leg():
    rec = _bench(["--full", "--no-cpu-baseline", "--no-other-configs"])
    assert all(k in rec for k in HEADLINE), sorted(rec)
    assert rec["roofline"]["bound"] == "mfma" and rec["roofline"]["kernel"].endswith("<*>") and 0 < rec["roofline"]["frac"] < 1
    assert "cpu_baseline" not in rec and "other_configs" not in rec
