"""The SNR strip of the finishing column pass (csrc/pair_route.h fin_strip) on the host (tests/host): its pieces, the partition of its
samples over the column blocks' layout, the finisher's containment rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_fin_strip.cpp")
INC = os.path.join(ROOT, "pyaudiolocalization_amd", "csrc")


def _build_and_run(exe, flags):
    subprocess.run(["hipcc", "-O2", *flags, "-I", INC, SRC, "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fin_strip_geometry(tmp_path):
    """Pieces of the strip for n = 22873, 17075, 16385 and 88199 (lag windows clipped at either end, a window as wide as the row: no
    strip); every sample of the strip stored by exactly one (block, wavefront, slot, lane) of the Rader-89, dense and strips layouts
    and no other sample; the containment rule at win_lo, win_hi, one outside either, 0, n - 1 and the end pieces' borders."""
    res = _build_and_run(tmp_path / "test_fin_strip", [])
    assert "ALL OK" in res.stdout, res.stdout + res.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fin_strip_geometry_under_sanitizers(tmp_path):
    """the same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer (host code only)"""
    res = _build_and_run(tmp_path / "test_fin_strip_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
