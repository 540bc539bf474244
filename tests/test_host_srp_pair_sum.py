"""srp_pair_sum (csrc/srp_cells.h), the one body under k_srp_map, k_srp_zoom, k_srp_doa and k_srp_doa_zoom, compiled for the CPU
(tests/host/test_srp_pair_sum.cpp, with the address and undefined-behaviour sanitizers, -ffp-contract=off) against srp.py: both steers
(distances to a point, negated advances of a direction) times both terms (nearest lag, blended), at lanes 0 and 255 of a 16 x 256
column, M = 2 (one pair), 16 (one full tile), 17 (the first microphone of a second tile) and 33 (three tiles), with and without
weights, with T = half_width (nothing clips) and T = 3 (some terms clip).  Power bit for bit, clip counts exactly.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import srp_cases as S
import srp_doa_cases as D
import srp_zoom_cases as Z
from pyaudiolocalization_amd import srp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICS = [2, 16, 17, 33]
GRID = (2, 3, 5)
DOA_GRID = (3, 5)
LEVEL_Z = 4
T_CLIPS = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("srp_pair_sum") / "test_srp_pair_sum"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_srp_pair_sum.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, tmp_path, far, blended, t, mics, points, strips, weights):
    head = [float(far), float(blended), mics.shape[0], t, points.shape[0], float(weights is not None), S.MAP_FS, S.C_SOUND]
    parts = [head, mics, points, strips] + ([weights] if weights is not None else [])
    np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in parts]).tofile(tmp_path / "in.bin")
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr
    got = np.fromfile(tmp_path / "out.bin").reshape(2, points.shape[0], 2)
    assert got[0].tobytes() == got[1].tobytes()                                       # a lane's answer does not depend on its column
    return got[0, :, 0], got[0, :, 1].astype(np.int64)


def _check(got, power, clipped, t, m):
    assert got[0].tobytes() == np.ascontiguousarray(power, dtype=np.float64).tobytes()
    assert np.array_equal(got[1], clipped)
    if t != T_CLIPS:
        assert int(np.sum(clipped)) == 0                                              # half_width clips nothing
    elif m > 2:
        assert 0 < int(np.sum(clipped)) < clipped.shape[0] * (m * (m - 1) // 2)       # some terms clip, some are read


def _tile_sum(v, m):
    acc = np.zeros(v.shape[0])
    for p in srp.tile_order(m):
        acc = acc + v[:, p]
    return acc


def _cases(m):
    mics = S.map_mics(m)
    return mics, (srp.half_width(mics, S.MAP_FS, S.C_SOUND), T_CLIPS)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", MICS)
def test_near_nearest_equals_srp_map(exe, tmp_path, m, weighted):
    """srp.srp_map adds in pair order, the body in tile order: integer strips and weights make every order exact."""
    mics, ts = _cases(m)
    points = S.grid_of(GRID)
    for t in ts:
        st = S.integer_strips(m, t, 1)[0]
        wt = S.integer_weights(m, 1)[0] if weighted else None
        power, total = srp.srp_map(st, t, mics, S.MAP_FS, S.C_SOUND, S.MAP_LO, S.MAP_HI, GRID, wt)
        clipped = np.count_nonzero(~(np.abs(srp.lag_values(points, mics, S.MAP_FS, S.C_SOUND)) <= t), axis=1)
        assert int(np.sum(clipped)) == total
        _check(_run(exe, tmp_path, False, False, t, mics, points, st, wt), power, clipped, t, m)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", MICS)
def test_near_blended_equals_zoom_terms(exe, tmp_path, m, weighted):
    mics, ts = _cases(m)
    points = S.grid_of(GRID)
    for t in ts:
        st = Z.real_strips(m, t, 1)[0]
        wt = Z.real_weights(m, 1)[0] if weighted else None
        v, out, _, _, _ = srp.zoom_terms(st, t, points, mics, S.MAP_FS, S.C_SOUND, wt)
        _check(_run(exe, tmp_path, False, True, t, mics, points, st, wt), _tile_sum(v, m), np.count_nonzero(out, axis=1), t, m)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", MICS)
def test_far_nearest_equals_doa_map(exe, tmp_path, m, weighted):
    mics, ts = _cases(m)
    az, el, _ = D.axes(*DOA_GRID)
    points = srp.doa_directions(az, el)
    for t in ts:
        st = Z.real_strips(m, t, 1)[0]
        wt = Z.real_weights(m, 1)[0] if weighted else None
        power, total = srp.doa_map(st, t, mics, S.MAP_FS, S.C_SOUND, az, el, wt)
        clipped = np.count_nonzero(~(np.abs(np.rint(srp.doa_lag_quotients(points, mics, S.MAP_FS, S.C_SOUND))) <= t), axis=1)
        assert int(np.sum(clipped)) == total
        _check(_run(exe, tmp_path, True, False, t, mics, points, st, wt), power, clipped, t, m)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", MICS)
def test_far_blended_equals_doa_zoom_level(exe, tmp_path, m, weighted):
    mics, ts = _cases(m)
    for t in ts:
        st = Z.real_strips(m, t, 1)[0]
        wt = Z.real_weights(m, 1)[0] if weighted else None
        power, total, _, points = srp.doa_zoom_level(st, t, mics, S.MAP_FS, S.C_SOUND, D.AXIS_SEEDS[6], D.HALF0, LEVEL_Z, wt)
        out = srp.terms_at(st, t, srp.doa_lag_quotients(points, mics, S.MAP_FS, S.C_SOUND))[1]
        clipped = np.count_nonzero(out, axis=1)
        assert int(np.sum(clipped)) == total
        _check(_run(exe, tmp_path, True, True, t, mics, points, st, wt), power, clipped, t, m)
