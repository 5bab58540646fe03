"""bench.py's command line: the extra legs (roofline, cpu_baseline, other_configs) run only under --full."""
import sys


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.gpus, a.steps, a.warmup, a.dump_outputs) == (False, 1, 3, 1, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full and a.no_cpu_baseline and not a.no_roofline and not a.no_other_configs
