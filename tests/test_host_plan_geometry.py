"""The plan decision (csrc/plan_geometry.h) on the host: pins, invariants of every frame length, the table recorded from the
device, and length -> plan -> route (tests/host/test_plan_geometry.cpp)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "plan_table.json")


def flatten(table):
    """the fixture as lines '<set> <L> n conv_len m1 m2 n1 n2 tile_len'"""
    assert table["fields"] == ["n", "conv_len", "m1", "m2", "n1", "n2", "tile_len"]
    return "".join(f"{name} {length} {' '.join(str(int(v)) for v in row)}\n"
                   for name, rows in table["sets"].items() for length, row in rows.items())


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_plan_geometry_pins_invariants_and_recorded_table(tmp_path):
    """conv_geometry() / pfa_split() give the plans the GPU tests pin; for every frame length up to 2^20 and every plan switch both
    convolutions hold their sequence in whole tiles of a geometry the launch switches dispatch, and a cut is a coprime odd
    factorisation with consistent CRT constants, tile and chunks; 2^22 + 1 points are refused; the Rader index tables of 991 are
    permutations in mixed_radix.h's positions; every row of the table recorded from the device before the decision moved to the
    host is reproduced; and the plans give test_gpu_peak_positions.py's routes through pair_route()."""
    with open(TABLE) as fh:
        lines = flatten(json.load(fh))
    flat = tmp_path / "plan_table.txt"
    flat.write_text(lines)
    exe = tmp_path / "test_plan_geometry"
    subprocess.run(["hipcc", "-O2", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_plan_geometry.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(flat)], capture_output=True, text=True).stdout
    assert "ALL OK" in out, out
