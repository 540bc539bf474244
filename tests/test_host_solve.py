"""The batched position solve on the host: csrc/solve_math.h compiled for the CPU (tests/host/test_solve_math.cpp) and the NumPy
specification (pyaudiolocalization_amd/solve.py) on the reference's fixtures.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cases
from pyaudiolocalization_amd import pair_list
from pyaudiolocalization_amd import solve as S
from pyaudiolocalization_amd.utils import compute_weights, dynamic_bounds_extended, residuals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("solve_math") / "test_solve_math"
    subprocess.run(["hipcc", "-O2", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_solve_math.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, mode, array, tmp_path):
    path = tmp_path / f"{mode}.bin"
    np.ascontiguousarray(array, dtype=np.float64).tofile(path)
    return subprocess.run([exe, mode, str(path)], capture_output=True, text=True, check=True).stdout.split()


def test_damped_solve_held_coordinates_box_and_grid(exe):
    """3 x 3 damped solve against a long-double elimination (held coordinates: zero step), an indefinite matrix refused, the box
    and the grid's cell centres."""
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True).stdout
    assert "ALL OK" in out, out


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, 130, 257, 1000, 2016, 32640])
def test_pairwise_sum_is_numpys(exe, tmp_path, n):
    """snr / mean(snr) must equal utils.compute_weights bit for bit, so the mean is summed in NumPy's pairwise order."""
    x = np.random.default_rng(n).lognormal(1.0, 2.0, n)
    got = float.fromhex(_run(exe, "npsum", x, tmp_path)[0])
    assert got == float(np.sum(x))
    pairs = [tuple(p) for p in pair_list(64)][:n] if n <= 2016 else None
    if pairs is not None and len(pairs) == n:
        want = compute_weights({p: {"snr": s} for p, s in zip(pairs, x)}, pairs)
        assert np.array_equal(x / (got / n), want)
        assert np.array_equal(S.snr_weights(x), want)


@pytest.mark.parametrize("p", [6, 28, 2016, 32640])
def test_percentile_and_box(exe, tmp_path, p):
    rng = np.random.default_rng(p)
    td = rng.normal(0, 2e-3, p)
    td[rng.integers(0, p, p // 3)] = td[0]                      # ties, also around the 75 % rank
    td = np.round(td * 48000) / 48000
    v = cases.C_SOUND * np.abs(td)
    want = np.percentile(v, 75)
    got = float.fromhex(_run(exe, "pct", v, tmp_path)[0])
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(S.percentile75(v) - want) <= 1e-12 * abs(want)
    mics = rng.uniform(-2, 3, (9, 3))
    for buffer in (5.0, 0.0):
        lo, hi = S.box(mics, td, cases.C_SOUND, buffer)
        ref = dynamic_bounds_extended(mics, td, cases.C_SOUND, buffer=buffer)
        assert np.allclose(lo, [b[0] for b in ref], rtol=1e-12, atol=0) and np.allclose(hi, [b[1] for b in ref], rtol=1e-12, atol=0)


def _tdoa_inputs(golden):
    """(name, mics, k_sel, L, fs, calib, weights, snr, reference position): the tables of tests/test_host_tail.py."""
    g1, g2, g3, gx = (golden(n) for n in ("c1_example1.npz", "c2_chirp8.npz", "c3_grid64_trial0.npz", "localize_extras.npz"))
    out = [("c1", np.array(cases.c1_config()["mic_positions"]), g1["k_sel_0p05"], int(g1["L"][0]), 44100, None, "ones", None, g1["position"])]
    m2 = np.array(cases.c2_config()["mic_positions"])
    for tag in ("a_", "b_"):
        out.append(("c2" + tag, m2, g2[tag + "k_sel_0p05"], int(g2[tag + "L"][0]), 48000, None, "ones", None, g2[tag + "position"]))
    out.append(("c3", cases.grid_array_64(), g3["k_sel_0p05"], int(g3["L"][0]), 48000, None, "ones", None, g3["position"]))
    cfg = cases.loc_config(False)
    mx = np.array(cfg["mic_positions"])
    cal = np.array([d["delay"] for d in cases.LOC_CALIBRATION])
    k, length = gx["loc_k_sel_0p05"], int(gx["loc_L"][0])
    out.append(("extras plain", mx, k, length, cfg["fs"], None, "ones", None, gx["loc_position_plain"]))
    out.append(("extras calibrated", mx, k, length, cfg["fs"], cal, "ones", None, gx["loc_position_calib"]))
    out.append(("extras snr", mx, k, length, cfg["fs"], cal, "snr", gx["loc_snr"], gx["loc_position_metrics"]))
    return out


def fixture_cost(x, mics, k_sel, length, fs, calib, weights, snr):
    m = len(mics)
    pairs = [tuple(p) for p in pair_list(m)]
    td = [(np.int64(k) - (length - 1)) / fs for k in k_sel]
    if calib is not None:
        td = [t - (calib[j] - calib[i]) for t, (i, j) in zip(td, pairs)]
    w = None if weights == "ones" else compute_weights({p: {"snr": s} for p, s in zip(pairs, snr)}, pairs)
    return 0.5 * float(np.sum(residuals(x, mics, pairs, td, cases.C_SOUND, w) ** 2))


def test_specification_is_at_least_as_converged_as_the_reference(golden):
    """Cost at the returned position <= cost at the reference's own position (utils.residuals, margin 1e-9 relative: the reference
    stops at ftol 1e-6), and the winner ended inside a stop rule before the cap."""
    for name, mics, k_sel, length, fs, calib, weights, snr, ref in _tdoa_inputs(golden):
        rec = S.solve_frame(k_sel, length, mics, fs, cases.C_SOUND, calib, weights, snr)
        got = fixture_cost(rec["position"], mics, k_sel, length, fs, calib, weights, snr)
        want = fixture_cost(ref, mics, k_sel, length, fs, calib, weights, snr)
        print(f"{name}: cost {got:.9g} (reference {want:.9g}), start {rec['start']}, {rec['iterations']} trial points, "
              f"{rec['converged_starts']} of 65 starts converged, |position - reference| {np.max(np.abs(rec['position'] - ref)):.3g} m")
        assert got <= want * (1 + 1e-9), name
        assert rec["status"] & S.ST_CONVERGED and not rec["status"] & S.ST_HIT_CAP, name
        assert rec["iterations"] < S.MAX_ITER, name
        assert abs(rec["cost"] - got) <= 1e-9 * got, name


def test_header_iteration_follows_the_specification(exe, tmp_path, golden):
    """lm_solve of solve_math.h (sums in pair order) against solve.lm_solve from the same starts."""
    name, mics, k_sel, length, fs, calib, weights, snr, ref = _tdoa_inputs(golden)[1]
    td = S.time_delays(k_sel, length, fs, calib, len(mics))
    w = np.ones(td.shape[0])
    b = (cases.C_SOUND * td) * w
    lo, hi = S.box(mics, td, cases.C_SOUND)
    pi, pj = S.pair_indices(len(mics))
    for x0 in S.start_points(mics, lo, hi)[[0, 1, 22, 64]]:
        want = S.lm_solve(x0, lo, hi, mics, pi, pj, b, w)
        out = _run(exe, "lm", np.concatenate([[len(mics), td.shape[0], S.MAX_ITER], lo, hi, x0, mics.ravel(), b, w]), tmp_path)
        x, cost = np.array([float(v) for v in out[:3]]), float(out[3])
        assert int(out[5]) != S.STOP_CAP and want[3] != S.STOP_CAP
        assert abs(cost - want[1]) <= 1e-9 * want[1]
        assert np.max(np.abs(x - want[0])) <= 1e-6


def test_bad_weights_and_the_position_record_layout():
    assert [S.POSITION.fields[k][1] for k in ("position", "cost", "lower", "upper", "start", "iterations", "converged_starts", "status")] \
        == [0, 24, 32, 56, 80, 84, 88, 92]
    mics = np.array(cases.c1_config()["mic_positions"])
    snr = np.array([3.0, 4.0, np.inf, 2.0, 5.0, 1.0])
    rec = S.solve_frame(np.full(6, 44099), 44100, mics, 44100, cases.C_SOUND, weights="snr", snr=snr)
    assert rec["status"] == S.ST_BAD_WEIGHTS and np.all(np.isnan(rec["position"]))
