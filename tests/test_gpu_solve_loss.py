"""Robust losses of the device position solve (pal_solve_positions_loss*, csrc/solve.hip) on the outlier tables of
tests/robust_tables.py: batch invariance, SciPy's cost and polished point, the recovered source, the pair weights, the unchanged
linear path, the stream and the argument checks."""
import ctypes as C_

import numpy as np
import pytest

import robust_tables as T
from oracle import cases
from pyaudiolocalization_amd import _ffi
from pyaudiolocalization_amd import solve as S
from test_host_solve import _tdoa_inputs
from test_host_solve_loss import POSITION_BOUND

pytestmark = pytest.mark.gpu

ALL_CASES = T.CASES + T.SHAPE_CASES
# One call holds one microphone array, so the eight cases are batched per array (m, seed): each array's tables, repeated in turn
# until the call has B = 8 frames.
ARRAYS = sorted({case[:2] for case in ALL_CASES})
KW = dict(weights="ones", buffer=T.BUFFER, grid=T.GRID)


def _solve(engine, case_list, **kw):
    tabs = np.stack([T.table(*case)["records"] for case in case_list])
    return engine.solve_positions(tabs, T.LENGTH, T.table(*case_list[0])["mics"], T.FS, T.C_SOUND, **KW, **kw)


@pytest.fixture(scope="module")
def single(engine):
    """One frame per call: {(case, loss): record}, linear (through the existing symbol) included."""
    return {(case, loss): _solve(engine, [case], **({} if loss == "linear" else dict(loss=loss, f_scale=T.F_SCALE)))[0]
            for case in ALL_CASES for loss in ("linear",) + T.ROBUST}


@pytest.mark.parametrize("loss", T.ROBUST)
def test_batch_invariance_cost_and_polished_point(engine, single, loss):
    for array in ARRAYS:
        group = [case for case in ALL_CASES if case[:2] == array]
        batch = [group[k % len(group)] for k in range(8)]
        recs = _solve(engine, batch, loss=loss, f_scale=T.F_SCALE)
        for case, rec in zip(batch, recs):
            assert rec.tobytes() == single[case, loss].tobytes(), (case, "batch of 8 against one frame per call")
    for case in ALL_CASES:
        rec = single[case, loss]
        want, _ = T.scipy_best(*case, loss)
        dist = float(np.linalg.norm(T.scipy_polish(*case, loss, rec["position"]) - rec["position"]))
        print(f"[solve loss] {case} {loss}: cost {rec['cost']:.15g}, SciPy {want:.15g}, excess {(rec['cost'] - want) / want:.3g}; "
              f"|position - SciPy restarted there| {dist:.3g} m; start {rec['start']}, {rec['iterations']} trial points, "
              f"{rec['converged_starts']} of 65 converged")
        assert rec["status"] & S.ST_CONVERGED and not rec["status"] & S.ST_HIT_CAP, case
        assert rec["cost"] <= want * (1 + 1e-9), case
        assert dist <= POSITION_BOUND, case


def test_cauchy_recovers_the_source_where_linear_is_metres_off(single):
    for case in T.OUTLIER_CASES:
        assert np.linalg.norm(single[case, "cauchy"]["position"] - T.SRC) < 0.15, case
        assert np.linalg.norm(single[case, "linear"]["position"] - T.SRC) > 1.0, case
    for loss in ("linear",) + T.ROBUST:
        assert np.linalg.norm(single[(8, 2, 0), loss]["position"] - T.SRC) < 0.01, loss


@pytest.mark.parametrize("case", [(8, 2, 4), (16, 3, 30)])
def test_pair_weights(engine, single, case):
    t = T.table(*case)
    rec, w = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, **KW, loss="cauchy", f_scale=T.F_SCALE,
                                    return_pair_weights=True)
    assert rec.tobytes() == single[case, "cauchy"].tobytes()                     # asking for the weights changes no record
    assert w.shape == (1, t["records"].shape[0])
    far = t["bad"][np.abs(t["lag"] - t["true_lag"])[t["bad"]] > 50]
    kept = np.setdiff1d(np.arange(w.shape[1]), t["bad"])
    print(f"[solve loss] {case}: weights of the {far.size} replaced pairs <= {w[0, far].max():.3g}, of the {kept.size} kept pairs >= {w[0, kept].min():.3g}")
    assert far.size and np.all(w[0, far] < 0.1)
    assert np.all(w[0, kept] > 0.5)
    pi, pj = S.pair_indices(len(t["mics"]))
    b = T.C_SOUND * S.time_delays(t["k_sel"], T.LENGTH, T.FS)
    want = S.pair_weights(rec["position"][0], t["mics"], pi, pj, b, np.ones(b.shape[0]), "cauchy", T.F_SCALE)
    assert np.allclose(w[0], want, rtol=1e-9, atol=0)                            # rho'(z) = 1 / (1 + z): a few roundings of z
    rec, w = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, **KW, return_pair_weights=True)
    assert np.array_equal(w, np.ones_like(w)) and rec.tobytes() == single[case, "linear"].tobytes()


def _raw(engine, symbol, tab, mics, length, fs, c, loss, f_scale, pw=None):
    """The C ABI itself: pal_solve_positions_loss with ones for weights, the default grid and box -> (return code, records)."""
    tab = np.ascontiguousarray(tab)
    b, p = tab.shape
    mics = np.ascontiguousarray(mics, dtype=np.float64)
    ln = np.full(b, length, dtype=np.int32)
    prm = _ffi.SolveParams(float(fs), float(c), T.BUFFER, T.GRID, S.MAX_ITER, S.WEIGHTS["ones"], 0)
    out = np.zeros(b, dtype=S.POSITION)
    rc = getattr(engine._lib, symbol)(engine._h, tab.ctypes.data, b, mics.shape[0], ln.ctypes.data, mics.ctypes.data, None, None, None,
                                      C_.byref(prm), out.ctypes.data, loss, f_scale, _ffi.ptr(pw))
    return rc, out


def test_linear_through_the_new_symbols_is_the_existing_solve(engine, single, golden):
    for case in ALL_CASES:
        t = T.table(*case)
        pw = np.zeros((1, t["records"].shape[0]))
        rc, out = _raw(engine, "pal_solve_positions_loss", t["records"][None], t["mics"], T.LENGTH, T.FS, T.C_SOUND, S.LOSSES["linear"], T.F_SCALE, pw)
        assert rc == 0 and out[0].tobytes() == single[case, "linear"].tobytes(), case
        assert np.array_equal(pw, np.ones_like(pw))
    name, mics, k_sel, length, fs, calib, weights, snr, _ = _tdoa_inputs(golden)[3]          # the C3 table: 2016 pairs
    tab = np.zeros((1, len(k_sel)), dtype=_ffi.RECORD)
    tab["k_sel"] = k_sel
    tab["snr"] = 1.0
    want = engine.solve_positions(tab, length, mics, fs, cases.C_SOUND)
    rc, out = _raw(engine, "pal_solve_positions_loss", tab, mics, length, fs, cases.C_SOUND, S.LOSSES["linear"], 1.0)
    assert rc == 0 and out.tobytes() == want.tobytes(), name
    got, pw = engine.solve_positions(tab, length, mics, fs, cases.C_SOUND, loss="linear", f_scale=0.3, return_pair_weights=True)
    assert got.tobytes() == want.tobytes() and np.array_equal(pw, np.ones_like(pw))
    d_tab = engine.alloc(tab.nbytes)
    try:
        engine.upload(d_tab, tab)
        dev = engine.solve_positions_dev(d_tab, 1, length, mics, fs, cases.C_SOUND, loss="linear", return_pair_weights=True)[0]
        assert dev.tobytes() == want.tobytes()
        t = T.table(16, 3, 30)
        engine.upload(d_tab, t["records"])
        dev = engine.solve_positions_dev(d_tab, 1, T.LENGTH, t["mics"], T.FS, T.C_SOUND, **KW, loss="huber", f_scale=T.F_SCALE)
        assert dev[0].tobytes() == single[(16, 3, 30), "huber"].tobytes()                      # tables in HBM: the same records
    finally:
        engine.free(d_tab)


def test_position_stream_with_a_loss(engine):
    from pyaudiolocalization_amd.stream import position_stream
    from test_gpu_stream import _c5_like_frames
    bases, delays, gains, totals, trim, fs = _c5_like_frames(7)
    pos = np.random.default_rng(55).uniform(-0.4, 0.4, (8, 3))           # the array of _c5_like_frames
    c = cases.C_SOUND
    p1, t1, l1 = position_stream(bases, delays, gains, fs, totals, trim, pos, c, "butterworth", 0.05, engine=engine, frames_per_batch=4)
    p2, t2, l2 = position_stream(bases, delays, gains, fs, totals, trim, pos, c, "butterworth", 0.05, engine=engine, frames_per_batch=4,
                                 loss="cauchy", f_scale=0.05)
    assert t2.tobytes() == t1.tobytes() and np.array_equal(l2, l1)
    assert p2.tobytes() == engine.solve_positions(t2, l2, pos, fs, c, loss="cauchy", f_scale=0.05).tobytes()
    assert p1.tobytes() == engine.solve_positions(t1, l1, pos, fs, c).tobytes()


def test_argument_errors(engine):
    t = T.table(4, 5, 1)
    for kw in (dict(loss="l2"), dict(loss=None), dict(loss="cauchy", f_scale=0.0), dict(loss="cauchy", f_scale=-0.05),
               dict(loss="huber", f_scale=float("nan")), dict(loss="soft_l1", f_scale=float("inf")), dict(loss="linear", f_scale=0.0)):
        with pytest.raises(ValueError):
            engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, **kw)
        with pytest.raises(ValueError):
            engine.solve_positions_dev(0, 1, T.LENGTH, t["mics"], T.FS, T.C_SOUND, **kw)
    d_tab = engine.alloc(t["records"].nbytes)
    try:
        engine.upload(d_tab, t["records"])
        for symbol, tab in (("pal_solve_positions_loss", t["records"][None]), ("pal_solve_positions_loss_dev", None)):
            for loss, f_scale in ((-1, 0.05), (4, 0.05), (3, 0.0), (3, -0.05), (1, float("nan")), (2, float("inf")), (0, 0.0), (0, float("nan"))):
                if tab is not None:
                    rc, _ = _raw(engine, symbol, tab, t["mics"], T.LENGTH, T.FS, T.C_SOUND, loss, f_scale)
                else:
                    mics = np.ascontiguousarray(t["mics"])
                    ln = np.full(1, T.LENGTH, dtype=np.int32)
                    prm = _ffi.SolveParams(T.FS, T.C_SOUND, T.BUFFER, T.GRID, S.MAX_ITER, 0, 0)
                    out = np.zeros(1, dtype=S.POSITION)
                    rc = engine._lib.pal_solve_positions_loss_dev(engine._h, C_.c_void_p(d_tab), 1, 4, ln.ctypes.data, mics.ctypes.data, None, None,
                                                                  None, C_.byref(prm), out.ctypes.data, loss, f_scale, None)
                assert rc == _ffi.ERR_INVALID, (symbol, loss, f_scale)
    finally:
        engine.free(d_tab)
