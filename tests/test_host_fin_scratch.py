"""Layout and reset rule of the finishing pass's per-stream scratch block (csrc/fin_scratch.h), on the host (tests/host)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fin_scratch_layouts_and_reset_rule(tmp_path):
    """Regions aligned and disjoint; a layout's `done` words can lie on another layout's maxima / partials (the hazard, on
    record); the block is zeroed on every layout change and at the wrap, never for the same layout below the bound; a slot
    driven through every ordered pair of layouts and across the wrap never trusts a word another layout or cycle wrote."""
    exe = tmp_path / "test_fin_scratch"
    subprocess.run(["hipcc", "-O2", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_fin_scratch.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    assert "ALL OK" in out, out
