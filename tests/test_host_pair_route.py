"""The route of a pair-pipeline call (csrc/pair_route.h) against a restatement of its rules, on the host (tests/host)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_pair_route_matches_the_rules(tmp_path):
    """pair_route() equals the chain of booleans pair_correlations once computed, over the plan shapes of the GPU cases x
    every combination of the switches, table / corr / multi / stored-only, num_peaks, method, multiplier and pair count; the
    routes the GPU tests expect are pinned by name; a stored-rows-only call never takes a route that flags pairs."""
    exe = tmp_path / "test_pair_route"
    subprocess.run(["hipcc", "-O2", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_pair_route.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    assert "ALL OK" in out, out
