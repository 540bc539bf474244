"""Robust losses of the position solve on the host: the NumPy specification (pyaudiolocalization_amd/solve.py, loss= / f_scale=)
against SciPy's least_squares on the outlier tables of tests/robust_tables.py, the unchanged linear path, and the loss
functions of csrc/solve_math.h compiled for the CPU with the address and undefined-behaviour sanitizers
(tests/host/test_solve_loss.cpp).  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import robust_tables as T
from oracle import cases
from pyaudiolocalization_amd import solve as S
from pyaudiolocalization_amd import stream
from test_host_solve import _tdoa_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# |specification's position - SciPy restarted there with tolerances 1e-15|: the largest distance observed over the six cases and
# three losses is 2.05e-7 m (huber on (16, 3, 30); next 1.5e-7 m, soft_l1 on (8, 11, 7); eleven of the eighteen are exactly 0).
# The bound is ten times that, well under the 1e-4 m cap (1 / 70 of the 7.16 mm of path one sample at 48 kHz is worth).
POSITION_BOUND = min(10 * 2.05e-7, 1e-4)


def spec(case, loss):
    t = T.table(*case)
    return S.solve_frame(t["k_sel"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="ones", buffer=T.BUFFER, grid=T.GRID, loss=loss,
                         f_scale=T.F_SCALE)


@pytest.fixture(scope="module")
def records():
    return {(case, loss): spec(case, loss) for case in T.CASES for loss in ("linear",) + T.ROBUST}


@pytest.mark.parametrize("loss", T.ROBUST)
@pytest.mark.parametrize("case", T.CASES)
def test_cost_is_at_or_below_scipys_best(records, case, loss):
    rec = records[case, loss]
    want, _ = T.scipy_best(*case, loss)
    print(f"{case} {loss}: cost {rec['cost']:.15g}, SciPy's best of 65 starts {want:.15g}, relative excess {(rec['cost'] - want) / want:.3g}, "
          f"{rec['iterations']} trial points, {rec['converged_starts']} of 65 starts converged")
    assert rec["status"] & S.ST_CONVERGED and not rec["status"] & S.ST_HIT_CAP
    assert rec["cost"] <= want * (1 + 1e-9)
    residuals = T.problem(*case)[0]
    z = (residuals(rec["position"]) / T.F_SCALE) ** 2           # the record's cost is F at its position
    assert abs(rec["cost"] - 0.5 * T.F_SCALE ** 2 * float(np.sum(S.loss_terms(loss, z)[0]))) <= 1e-12 * rec["cost"]


@pytest.mark.parametrize("loss", T.ROBUST)
@pytest.mark.parametrize("case", T.CASES)
def test_position_is_scipys_polished_point(records, case, loss):
    rec = records[case, loss]
    dist = float(np.linalg.norm(T.scipy_polish(*case, loss, rec["position"]) - rec["position"]))
    print(f"{case} {loss}: |position - SciPy restarted there| = {dist:.3g} m")
    assert dist <= POSITION_BOUND


@pytest.mark.parametrize("case", T.OUTLIER_CASES)
def test_cauchy_recovers_the_source_where_linear_is_metres_off(records, case):
    err = {loss: float(np.linalg.norm(records[case, loss]["position"] - T.SRC)) for loss in ("linear", "cauchy")}
    print(f"{case}: {err}")
    assert err["cauchy"] < 0.15
    assert err["linear"] > 1.0


def test_all_losses_agree_on_a_clean_table(records):
    for loss in ("linear",) + T.ROBUST:
        assert np.linalg.norm(records[(8, 2, 0), loss]["position"] - T.SRC) < 0.01, loss


def test_linear_keyword_is_todays_path(golden):
    """loss='linear' (whatever f_scale) returns the records of the call without the keyword, byte for byte, on the C1, C2 and C3 fixtures."""
    for name, mics, k_sel, length, fs, calib, weights, snr, _ in _tdoa_inputs(golden)[:4]:
        want = S.solve_frame(k_sel, length, mics, fs, cases.C_SOUND, calib, weights, snr)
        got = S.solve_frame(k_sel, length, mics, fs, cases.C_SOUND, calib, weights, snr, loss="linear", f_scale=0.05)
        assert got.tobytes() == want.tobytes(), name
    td = S.time_delays(k_sel, length, fs, calib, len(mics))
    pi, pj = S.pair_indices(len(mics))
    w = np.ones(td.shape[0])
    lo, hi = S.box(mics, td, cases.C_SOUND)
    x0 = S.start_points(mics, lo, hi)[5]
    a = S.lm_solve(x0, lo, hi, mics, pi, pj, cases.C_SOUND * td, w)
    b = S.lm_solve(x0, lo, hi, mics, pi, pj, cases.C_SOUND * td, w, loss="linear", f_scale=3.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


@pytest.mark.parametrize("loss,f_scale", [("l2", 1.0), (None, 1.0), (2, 1.0), ("cauchy", 0.0), ("cauchy", -0.05), ("huber", float("nan")),
                                          ("soft_l1", float("inf")), ("linear", 0.0), ("cauchy", "wide")])
def test_bad_loss_arguments_raise_before_any_gpu_work(loss, f_scale):
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was reached before the argument checks")

    t = T.table(4, 5, 1)
    with pytest.raises(ValueError):
        S.check_loss(loss, f_scale)
    with pytest.raises(ValueError):
        S.solve_frame(t["k_sel"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, loss=loss, f_scale=f_scale)
    rows = np.random.default_rng(5).standard_normal((3, 1200))
    with pytest.raises(ValueError):
        stream.recorded_position_stream(rows, 12000.0, 8000.0, 400, 200, t["mics"][:3], 343.0, engine=NoEngine(), loss=loss, f_scale=f_scale)
    with pytest.raises(ValueError):
        stream.position_stream([], [], [], T.FS, [], 100, t["mics"], 343.0, engine=NoEngine(), loss=loss, f_scale=f_scale)


def test_pair_weights_of_the_specification():
    case = (8, 2, 4)
    t = T.table(*case)
    pi, pj = S.pair_indices(8)
    b = T.C_SOUND * S.time_delays(t["k_sel"], T.LENGTH, T.FS)
    ones = np.ones(b.shape[0])
    x = spec(case, "cauchy")["position"]
    w = S.pair_weights(x, t["mics"], pi, pj, b, ones, "cauchy", T.F_SCALE)
    far = t["bad"][np.abs(t["lag"] - t["true_lag"])[t["bad"]] > 50]
    kept = np.setdiff1d(np.arange(b.shape[0]), t["bad"])
    assert far.size and np.all(w[far] < 0.1) and np.all(w[kept] > 0.5)
    assert np.array_equal(S.pair_weights(x, t["mics"], pi, pj, b, ones, "linear", T.F_SCALE), ones)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("solve_loss") / "test_solve_loss"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_solve_loss.cpp"), "-o", str(out)], check=True)
    return str(out)


def test_loss_functions_against_long_double(exe):
    """rho, rho' and rho' + 2 z rho'' within 4 ulp of long-double evaluations at z = 0, 1e-300, 1e-16, 1e-8, 0.5, 1 - 2^-52, 1,
    1 + 2^-52, 4, 1e8, 1e300; Huber's two branches at the seam."""
    run = subprocess.run([exe, "selftest"], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr


@pytest.mark.parametrize("loss", T.ROBUST)
def test_header_iteration_follows_the_specification(exe, tmp_path, loss):
    """lm_solve<kSumsLoss> of solve_math.h (sums in pair order) against solve.lm_solve from the same starts."""
    case = (8, 2, 4)
    t = T.table(*case)
    mics = t["mics"]
    b = T.C_SOUND * S.time_delays(t["k_sel"], T.LENGTH, T.FS)
    w = np.ones(b.shape[0])
    _, lo, hi, starts = T.problem(*case)
    pi, pj = S.pair_indices(len(mics))
    path = tmp_path / "lm.bin"
    for x0 in starts[[0, 1, 22, 64]]:
        want = S.lm_solve(x0, lo, hi, mics, pi, pj, b, w, loss=loss, f_scale=T.F_SCALE)
        np.concatenate([[len(mics), b.shape[0], S.MAX_ITER], lo, hi, x0, mics.ravel(), b, w]).tofile(path)
        run = subprocess.run([exe, "lm", loss, repr(T.F_SCALE), str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        out = run.stdout.split()
        x, cost = np.array([float(v) for v in out[:3]]), float(out[3])
        assert int(out[5]) != S.STOP_CAP and want[3] != S.STOP_CAP
        assert abs(cost - want[1]) <= 1e-9 * want[1]
        assert np.max(np.abs(x - want[0])) <= 1e-6
