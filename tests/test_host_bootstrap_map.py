"""csrc/bootstrap_map.h compiled for the CPU with the address and undefined-behaviour sanitizers against the specification
(pyaudiolocalization_amd/bootstrap.py): ShuffleMap's closed form at its degenerate shapes, the Feistel network and the cycle walk
against their inverses (tests/host/test_bootstrap_map.cpp; cases: tests/bootstrap_shapes.py).  No GPU."""
import os
import shutil
import subprocess

import pytest

import bootstrap_shapes as BS
from pyaudiolocalization_amd import bootstrap as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_lines():
    """'L i j s mode block_size seed digest' per case, followed by the L indices themselves where L <= 64"""
    for L, i, j, s, mode, bs, seed in BS.map_cases():
        idx = B.shuffle_indices(L, i, j, s, mode, bs, seed)
        tail = "".join(f" {int(v)}" for v in idx) if L <= 64 else ""
        yield f"{L} {i} {j} {s} {B.MODES[mode]} {bs} {seed} {BS.fnv1a64(idx)}{tail}\n"


def test_the_grid_holds_the_degenerate_shapes():
    cases = list(BS.map_cases())
    assert len(cases) >= 900 and len(set(cases)) == len(cases)
    block = {(L, bs) for L, _, _, _, mode, bs, _ in cases if mode == "block"}
    for L in BS.MAP_LENGTHS:
        assert {(L, 1), (L, L), (L, L + 1), (L, 2**31 - 1)} <= block                 # single samples, one block (three ways)
        assert L < 4 or any(bs < L and L % bs == 0 for l, bs in block if l == L)     # the 'short' block is full
        assert L < 4 or any(bs < L and L % bs == 1 for l, bs in block if l == L)     # ... and one sample long
    assert {(BS.MAP_LIMIT, 1), (BS.MAP_LIMIT, 50), (BS.MAP_LIMIT, BS.MAP_LIMIT)} <= block
    assert any(s >= 2**62 for _, _, _, s, _, _, _ in cases) and any(i == 2**31 - 1 for _, i, _, _, _, _, _ in cases)
    assert any(seed == 2**64 - 1 for *_, seed in cases)
    # lengths on both sides of 4^h: with and without cycle walking
    assert all({4**h - 1, 4**h, 4**h + 1} <= set(BS.MAP_LENGTHS) for h in range(1, 7))


def test_short_block_lands_first_and_last_within_the_device_tests_shuffles():
    """what tests/test_gpu_bootstrap_edges.py relies on, by the specification alone"""
    assert BS.SHORT_BLOCK_FIRST < BS.BLOCK_SHUFFLES and BS.SHORT_BLOCK_LAST < BS.BLOCK_SHUFFLES
    assert BS.short_block_position(1000, BS.SHORT_BLOCK_FIRST, 50) == 0
    assert BS.short_block_position(1000, BS.SHORT_BLOCK_LAST, 50) == 950


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_shuffle_map_equals_the_specification(tmp_path):
    """ShuffleMap(t), t = 0 .. L-1, equals shuffle_indices on every case of bootstrap_shapes.map_cases() (digest; element by element
    for L <= 64), and feistel_inv / walk_inv undo feistel / walk on n = 1, 2, 4, 5, 16, 17, 1024, 1025 under three keys."""
    flat = tmp_path / "map_cases.txt"
    flat.write_text("".join(case_lines()))
    exe = tmp_path / "test_bootstrap_map"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_bootstrap_map.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(flat)], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr
