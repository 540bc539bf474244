"""What the closure check and the consensus share on the device (csrc/closure_tiles.h) against plain loops, on the host (tests/host)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_closure_tiles_match_plain_loops(tmp_path):
    """pair_row enumerates the pairs i < j row by row for every M in 2..256 (and in 64 bits past int32), tile_of the tiles on and above the
    diagonal for 1..16 tiles per side; tile_votes<1> and tile_votes<4>, lane by lane on host arrays, equal a triple loop that skips k = i and
    k = j at M = 3, 16, 17, 33 with lags in +-40 and tol 0, 1, 5, and on triangles of the lags -(2^24 - 1), 0, 2^24 - 1 with tol 0 and 2^20;
    lag_of_index at k = -1, 0, 2L - 2 and 2L - 1."""
    exe = tmp_path / "test_closure_tiles"
    subprocess.run(["hipcc", "-O2", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_closure_tiles.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    assert "ALL OK" in out, out
