"""The batched device position solve (csrc/solve.hip, pal_solve_positions*) against its NumPy specification
(pyaudiolocalization_amd/solve.py), the reference's fixtures, SciPy with the same bounds, and through the Python layers."""
import numpy as np
import pytest
from scipy.optimize import least_squares

from oracle import cases
from pyaudiolocalization_amd import RECORD, pair_list
from pyaudiolocalization_amd import solve as S
from pyaudiolocalization_amd.utils import compute_weights, equations_jacobian, residuals

from test_host_solve import _tdoa_inputs, fixture_cost

pytestmark = pytest.mark.gpu

# |device - specification| per coordinate (the sums over the pairs run in another order): ten times the largest difference observed on
# the fixtures on an MI355X - 2.13e-7 m on C3; C1 2.4e-12, C2 6.0e-11, five-microphone table 4.4e-15 / 1.5e-14 / 5.3e-8 - and
# well inside a tenth of the project's 1e-3 m position bar (1e-4 m), the most it may ever be.  The first test prints every figure.
POSITION_TOL = 2.13e-6
assert POSITION_TOL <= 1e-4
C = cases.C_SOUND


@pytest.fixture(scope="module", autouse=True)
def _engine(engine):
    import pyaudiolocalization_amd.engine as E
    E._default = engine
    yield
    E._default = None


def _table(k_sel, snr=None):
    t = np.zeros(len(k_sel), dtype=RECORD)
    t["k_sel"] = k_sel
    t["snr"] = 1.0 if snr is None else snr
    return t


def _synthetic(mics, src, length, fs, noise, seed):
    rng = np.random.default_rng(seed)
    d = np.linalg.norm(mics - src, axis=1)
    pl = pair_list(len(mics))
    td = (d[pl[:, 1]] - d[pl[:, 0]]) / C + rng.normal(0, noise, len(pl))
    return _table(np.rint(td * fs).astype(np.int64) + (length - 1), rng.uniform(1, 9, len(pl)))


def _polished(x0, mics, k_sel, length, fs, calib, weights, snr):
    pairs = pair_list(len(mics))
    td = S.time_delays(k_sel, length, fs, calib, len(mics))
    w = np.ones(len(td)) if weights == "ones" else S.snr_weights(snr)
    lo, hi = S.box(mics, td, C)                                          # the reference solves inside this box (main.py:246-274); so does the polish
    return least_squares(residuals, np.clip(x0, lo, hi), jac=equations_jacobian, args=(mics, pairs, td, C, w), bounds=(lo, hi), method="trf",
                         ftol=1e-15, xtol=1e-15, gtol=1e-15).x


def test_fixtures_cost_specification_and_polished_reference(engine, golden):
    worst = 0.0
    for name, mics, k_sel, length, fs, calib, weights, snr, ref in _tdoa_inputs(golden):
        rec = engine.solve_positions(_table(k_sel, snr), length, mics, fs, C, calib, weights)[0]
        spec = S.solve_frame(k_sel, length, mics, fs, C, calib, weights, snr)
        got = fixture_cost(rec["position"], mics, k_sel, length, fs, calib, weights, snr)
        want = fixture_cost(ref, mics, k_sel, length, fs, calib, weights, snr)
        polished = _polished(ref, mics, k_sel, length, fs, calib, weights, snr)
        d_spec = float(np.max(np.abs(rec["position"] - spec["position"])))
        worst = max(worst, d_spec)
        print(f"[solve] {name}: cost {got:.9g} (reference {want:.9g}); |device - specification| {d_spec:.3g} m; "
              f"|device - reference| {np.max(np.abs(rec['position'] - ref)):.3g} m; |reference - polished| {np.max(np.abs(ref - polished)):.3g} m; "
              f"|device - polished| {np.max(np.abs(rec['position'] - polished)):.3g} m; start {rec['start']} ({spec['start']}), "
              f"{rec['iterations']} trial points, {rec['converged_starts']} starts converged")
        assert got <= want * (1 + 1e-9), name
        assert rec["status"] & S.ST_CONVERGED and not rec["status"] & S.ST_HIT_CAP, name
        assert d_spec <= POSITION_TOL, name
        assert np.max(np.abs(rec["position"] - polished)) <= POSITION_TOL, name
        assert np.array_equal(rec["lower"], spec["lower"]) and np.array_equal(rec["upper"], spec["upper"]), name
    print(f"[solve] largest |device - specification| {worst:.3g} m")


def test_the_box_binds(engine):
    mics = np.array(cases.c2_config()["mic_positions"], dtype=float)
    src = mics.mean(axis=0) + np.array([6.0, -1.0, 0.5])                 # outside: the box is the array's extent -/+ >= 1 m
    tab = _synthetic(mics, src, 12000, 48000.0, 0.0, 1)
    rec = engine.solve_positions(tab, 12000, mics, 48000.0, C, buffer=0.0)[0]
    lo, hi = rec["lower"], rec["upper"]
    x = rec["position"]
    assert not (lo[0] <= src[0] <= hi[0])
    assert np.all(x >= lo) and np.all(x <= hi)
    assert rec["status"] & S.ST_ON_FACE and rec["status"] & S.ST_CONVERGED
    assert np.any((x == lo) | (x == hi))
    pairs = pair_list(len(mics))
    td = S.time_delays(tab["k_sel"], 12000, 48000.0)
    # SciPy from five of the 65 starts (the centre, two opposite corners' cells and two inner cells): each run costs a second of host
    # time and on this table they all end in the same minimum on the face
    best = min((least_squares(residuals, s, jac=equations_jacobian, args=(mics, pairs, td, C, None), bounds=(lo, hi), method="trf").cost
                for s in S.start_points(mics, lo, hi)[[0, 1, 22, 43, 64]]))
    print(f"[solve] box: position {x}, cost {rec['cost']:.9g}, SciPy with the same bounds {best:.9g}")
    assert rec["cost"] <= best * (1 + 1e-9)
    spec = S.solve_frame(tab["k_sel"], 12000, mics, 48000.0, C, buffer=0.0)
    assert np.array_equal(lo, spec["lower"]) and np.array_equal(hi, spec["upper"])
    held = (spec["position"] == lo) | (spec["position"] == hi)
    assert held.any()
    assert np.array_equal(x[held], spec["position"][held])                # on the face exactly, not near it
    assert np.array_equal(held, (x == lo) | (x == hi))


@pytest.mark.parametrize("p_mics", [4, 8, 64, 256])                      # 6, 28, 2016 and 32 640 pairs
def test_box_is_dynamic_bounds_extended_with_ties(engine, p_mics):
    """The device's percentile (a radix select over the bit patterns) through the box it produces: tie-heavy tables whose 75th
    percentile of c |td| lies above 1 m, against utils.dynamic_bounds_extended (np.percentile) and the specification."""
    from pyaudiolocalization_amd.utils import dynamic_bounds_extended
    rng = np.random.default_rng(p_mics)
    mics = rng.uniform(-2, 3, (p_mics, 3))
    npairs = p_mics * (p_mics - 1) // 2
    fs, length = 48000.0, 24000
    for case in range(3):
        lag = rng.integers(-2400, 2401, npairs)                           # c |td| up to 17 m
        lag[rng.integers(0, npairs, npairs // 2)] = lag[0]                # half the table tied
        if case == 1:
            lag[:] = np.sort(np.abs(lag))[(3 * (npairs - 1)) // 4]        # every value equal
        if case == 2:
            lag = -np.abs(lag)
        tab = _table(lag + (length - 1))
        for buffer in (5.0, 0.0):
            rec = engine.solve_positions(tab, length, mics, fs, C, buffer=buffer, grid=1, max_iter=1)[0]
            td = S.time_delays(tab["k_sel"], length, fs)
            want = dynamic_bounds_extended(mics, td, C, buffer=buffer)
            lo, hi = S.box(mics, td, C, buffer)
            assert max(np.percentile(C * np.abs(td), 75), 1.0) > 1.0
            assert np.array_equal(rec["lower"], lo) and np.array_equal(rec["upper"], hi), (p_mics, case, buffer)
            assert np.allclose(rec["lower"], [b[0] for b in want], rtol=1e-12, atol=0)
            assert np.allclose(rec["upper"], [b[1] for b in want], rtol=1e-12, atol=0)


def test_batch_invariance(engine):
    mics = cases.grid_array_64()[:16]
    rng = np.random.default_rng(3)
    tabs = np.stack([_synthetic(mics, rng.uniform(-2, 2, 3), 9000 + 13 * f, 48000.0, 3e-5, 100 + f) for f in range(16)])
    lens = np.array([9000 + 13 * f for f in range(16)])
    together = engine.solve_positions(tabs, lens, mics, 48000.0, C, weights="snr")
    single = np.concatenate([engine.solve_positions(tabs[f], lens[f], mics, 48000.0, C, weights="snr") for f in range(16)])
    back = engine.solve_positions(tabs[::-1], lens[::-1], mics, 48000.0, C, weights="snr")[::-1]
    assert together.tobytes() == single.tobytes() == back.tobytes()
    assert np.all(together["status"] & S.ST_CONVERGED)


def test_256_microphones(engine):
    rng = np.random.default_rng(5)
    rng.normal(0, 2e-5, 2016)                                            # the draws of the 64-microphone half of the host test
    mics = cases.fibonacci_sphere(256, 0.5)
    pairs = pair_list(256)
    src = np.array([2.0, 1.0, 0.5])
    d = np.linalg.norm(mics - src, axis=1)
    td = np.array([(d[j] - d[i]) / C + rng.normal(0, 2e-5) for i, j in pairs])
    fs, length = 1e7, 100000                                             # a fine lag grid: the table carries td to 1e-7 s
    rec = engine.solve_positions(_table(np.rint(td * fs).astype(np.int64) + length - 1), length, mics, fs, C)[0]
    print(f"[solve] 256 microphones: |position - source| {np.max(np.abs(rec['position'] - src)):.3g} m, {rec['iterations']} trial points")
    assert rec["status"] & S.ST_CONVERGED
    assert np.max(np.abs(rec["position"] - src)) < 2e-2


def test_weights(engine, golden):
    from pyaudiolocalization_amd.main import host_position, solve_positions_device
    mics = cases.grid_array_64()
    tab = _synthetic(mics, np.array([0.7, -0.4, 1.3]), 12000, 48000.0, 2e-5, 9)
    pairs = [tuple(p) for p in pair_list(64)]
    w = compute_weights({p: {"snr": float(s)} for p, s in zip(pairs, tab["snr"])}, pairs)
    a = engine.solve_positions(tab, 12000, mics, 48000.0, C, weights="snr")
    b = engine.solve_positions(tab, 12000, mics, 48000.0, C, weights=w[None])
    assert a.tobytes() == b.tobytes()
    bad = tab.copy()
    bad["snr"][17] = np.inf
    rec = engine.solve_positions(bad, 12000, mics, 48000.0, C, weights="snr")[0]
    assert rec["status"] == S.ST_BAD_WEIGHTS and np.all(np.isnan(rec["position"]))
    # that frame goes to the host solve, whose answer to a weight that is not finite is SciPy's ValueError - in the SNR mode and, as
    # localize_sound_source passes them, with the weights as an array
    with pytest.raises(ValueError) as host_error:
        host_position(bad, 12000, mics, 48000.0, C, None, "snr")
    wbad = compute_weights({p: {"snr": float(s)} for p, s in zip(pairs, bad["snr"])}, pairs)
    for mode in ("snr", wbad[None]):
        with pytest.raises(ValueError) as device_error:
            solve_positions_device(bad, 12000, mics, 48000.0, C, weights=mode)
        assert str(device_error.value) == str(host_error.value)
    both = solve_positions_device(np.stack([tab, tab]), 12000, mics, 48000.0, C, weights="snr")
    assert np.array_equal(both[0], a[0]["position"]) and np.array_equal(both[1], a[0]["position"])


def test_position_stream(engine):
    from pyaudiolocalization_amd.stream import position_stream, tdoa_stream
    from test_gpu_stream import _c5_like_frames
    bases, delays, gains, totals, trim, fs = _c5_like_frames(7)
    pos = np.random.default_rng(55).uniform(-0.4, 0.4, (8, 3))           # the array of _c5_like_frames
    tables, lengths = tdoa_stream(bases, delays, gains, fs, totals, trim, "butterworth", 0.05, engine=engine, frames_per_batch=4)
    p2, t2, l2 = position_stream(bases, delays, gains, fs, totals, trim, pos, C, "butterworth", 0.05, engine=engine, frames_per_batch=4)
    assert t2.tobytes() == tables.tobytes() and np.array_equal(l2, lengths)
    assert p2.tobytes() == engine.solve_positions(tables, lengths, pos, fs, C).tobytes()


def test_localize_with_the_device_solver(engine, tmp_path, monkeypatch):
    from test_gpu_localize import _forced, _quiet
    import stages
    monkeypatch.chdir(tmp_path)
    M, filt = _forced(monkeypatch, stages.c2_case(False))
    host = M.localize_sound_source(_quiet(cases.c2_config()), use_simulation=True, show_plots=False)
    cfg = _quiet(cases.c2_config())
    cfg["localization"]["solver"] = "device"
    dev = M.localize_sound_source(cfg, use_simulation=True, show_plots=False)
    table = M.tdoa_table(filt, 48000, 0.05)
    mics = np.array(cfg["mic_positions"])
    polished = _polished(host["estimated_position"], mics, table["k_sel"], filt.shape[1], 48000, None, "ones", None)
    print(f"[solve] localize C2: |device - polished host| {np.max(np.abs(dev['estimated_position'] - polished)):.3g} m, "
          f"|host - polished host| {np.max(np.abs(host['estimated_position'] - polished)):.3g} m")
    assert np.max(np.abs(dev["estimated_position"] - polished)) <= POSITION_TOL
    assert sorted(dev) == sorted(host)
    cfg["localization"]["solver"] = "gpu"
    with pytest.raises(ValueError):
        M.localize_sound_source(cfg, use_simulation=True, show_plots=False)


def test_argument_errors(engine):
    mics = np.array(cases.c1_config()["mic_positions"], dtype=float)
    tab = _table(np.full(6, 44099))
    with pytest.raises(ValueError):
        engine.solve_positions(_table([]).reshape(1, 0), 44100, mics[:1], 44100, C)          # M = 1
    with pytest.raises(ValueError):
        engine.solve_positions(tab[:5], 44100, mics, 44100, C)                               # wrong table length
    with pytest.raises(ValueError):
        engine.solve_positions(tab, 44100, mics, 44100, C, grid=0)                           # no start beside the centre
    with pytest.raises(ValueError):
        engine.solve_positions(tab, 44100, mics, 0.0, C)                                     # fs <= 0
    ok = engine.solve_positions(tab, 44100, mics, 44100, C, grid=0, extra_starts=[[[0.2, 0.2, 0.2]]])
    assert ok["converged_starts"][0] == 2
