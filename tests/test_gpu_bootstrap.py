"""The device bootstrap (csrc/bootstrap.hip, pal_bootstrap_*): shuffles bit for bit against the NumPy specification
(pyaudiolocalization_amd/bootstrap.py), peaks against the oracle's PHAT of those shuffles, results keyed per pair (independent
of the pair list's order and of the round size), the null distribution of the reference's NumPy shuffles, and
localize_sound_source with localization.bootstrap_rng = "device" on the reference's fixture."""
import numpy as np
import pytest

from oracle import cases
from oracle import pal_oracle as O
from pyaudiolocalization_amd import bootstrap as B
from pyaudiolocalization_amd.engine import pair_list

import stages
from bootstrap_shapes import frame as _frame, oracle_peaks as _oracle_peaks

pytestmark = pytest.mark.gpu

MODES = ("permutation", "block", "circular")
TOL = dict(rtol=1e-10, atol=1e-13)            # the smoke test's tolerance on cmax


@pytest.fixture(scope="module", autouse=True)
def _engine(engine):
    import pyaudiolocalization_amd.engine as E
    E._default = engine
    yield
    E._default = None


@pytest.mark.parametrize("L", [1801, 44100])          # a prime length, and the prime-factor route's 44 100
@pytest.mark.parametrize("mode", MODES)
def test_shuffles_match_numpy(engine, L, mode):
    row = np.random.default_rng(L).standard_normal(L)
    S, s0, bs, seed = 9, 1000, 47, 2**63 + 12345        # 47 divides neither length; a seed above 2^63
    d_row = engine.alloc(row.nbytes)
    d_out = engine.alloc(S * row.nbytes)
    try:
        engine.upload(d_row, row)
        engine.bootstrap_shuffle_dev(d_row, L, 4, 9, mode, bs, seed, s0, S, d_out)
        engine.synchronize()
        got = engine.download(np.empty((S, L)), d_out)
    finally:
        engine.free(d_out)
        engine.free(d_row)
    for k in range(S):
        want = row[B.shuffle_indices(L, 4, 9, s0 + k, mode, bs, seed)]
        assert np.array_equal(got[k], want), (mode, L, k)


@pytest.mark.parametrize("mode", MODES)
def test_peaks_match_oracle_1800(engine, mode):
    rows, pairs = _frame(6, 1800), pair_list(6)
    got = engine.bootstrap_peaks(rows, pairs, 32, mode, 50, seed=3)
    assert got.shape == (15, 32)
    assert np.allclose(got, _oracle_peaks(rows, pairs, 32, mode, 50, 3), **TOL)


def test_peaks_match_oracle_44100(engine):
    rows, pairs = _frame(6, 44100), pair_list(6)
    got = engine.bootstrap_peaks(rows, pairs, 32, "permutation", 50, seed=4)
    assert np.allclose(got, _oracle_peaks(rows, pairs, 32, "permutation", 50, 4), **TOL)


def test_keyed_per_pair_not_per_position_or_round(engine):
    """A sub-list, the reversed list and rounds that split one pair's shuffles (pal_set_chunk) give the same peaks; only the
    last bits may differ (a pair's float fields depend on the pair packed beside it in one complex transform, DESIGN)."""
    rows, pairs = _frame(6, 1800), pair_list(6)
    close = dict(rtol=1e-11, atol=1e-15)
    for mode in ("permutation", "block"):
        full = engine.bootstrap_peaks(rows, pairs, 32, mode, 50, seed=8)
        sub = engine.bootstrap_peaks(rows, pairs[3:10], 32, mode, 50, seed=8)
        assert np.allclose(sub, full[3:10], **close)
        rev = engine.bootstrap_peaks(rows, pairs[::-1], 32, mode, 50, seed=8)
        assert np.allclose(rev[::-1], full, **close)
        try:
            engine.set_chunk(7)        # rounds of 56 shuffled rows: 480 = 8 x 56 + 32, every round splits a pair's 32 shuffles
            small = engine.bootstrap_peaks(rows, pairs, 32, mode, 50, seed=8)
            odd = engine.bootstrap_peaks(rows, pairs[2:], 31, mode, 50, seed=8)   # 403 = 7 x 56 + 11: an odd last round
        finally:
            engine.set_chunk(0)
        assert np.allclose(small, full, **close)
        assert np.allclose(odd, full[2:, :31], **close)
    assert not np.allclose(full, engine.bootstrap_peaks(rows, pairs, 32, "block", 50, seed=9), **close)


def test_all_zero_microphone(engine):
    rows = _frame(4, 1800)
    rows[2] = 0.0
    pairs = np.array([[0, 2], [2, 1], [0, 1], [3, 2]], dtype=np.int32)
    got = engine.bootstrap_peaks(rows, pairs, 6, "permutation", 50, seed=1)
    want = engine.gcc_phat_pairs(rows, pairs, 44100.0)["cmax"]
    for p in (0, 1, 3):
        np.testing.assert_array_equal(got[p], np.full(6, want[p]))   # (NaN included)
    assert np.all(np.isfinite(got[2]))


def _ks(a, b):
    a, b = np.sort(a), np.sort(b)
    x = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, x, side="right") / a.size - np.searchsorted(b, x, side="right") / b.size)))


def test_same_null_distribution_as_numpy_shuffles(engine):
    L, n = 4000, 2000
    g = np.random.default_rng(21)
    common = g.standard_normal(L + 40)
    a = common[20:20 + L] + g.standard_normal(L)
    b = common[27:27 + L] + g.standard_normal(L)
    dev = engine.bootstrap_peaks(np.stack([a, b]), [[0, 1]], n, "permutation", 50, seed=2024)[0]
    rng = np.random.default_rng(2025)
    host = np.concatenate([engine.gcc_phat_pairs(np.vstack([a[None], [rng.permutation(b) for _ in range(k)]]),
                                                 np.stack([np.zeros(k, np.int32), np.arange(1, k + 1, dtype=np.int32)], axis=1),
                                                 44100.0)["cmax"] for k in (1000, 1000)])
    d = _ks(dev, host)
    assert d < 0.062, d
    assert np.median(dev) < np.max(O.phat_correlation(a, b))      # the unshuffled pair stands far above its null


def test_thresholds_are_the_percentile_of_the_peaks(engine):
    from pyaudiolocalization_amd import utils as U
    rows, pairs = _frame(5, 1800), pair_list(5)
    for alpha in (0.05, 0.01):
        th = U.bootstrap_thresholds(rows, pairs, 44100.0, num_bootstrap=64, alpha=alpha, bootstrap_mode="circular", seed=6)
        peaks = engine.bootstrap_peaks(rows, pairs, 64, "circular", 50, seed=6)
        assert np.array_equal(th, np.percentile(peaks, 100 * (1 - alpha), axis=1))
    one = U.bootstrap_significance(rows[1], rows[3], 44100.0, num_bootstrap=64, rng="device", seed=6)
    assert one == np.percentile(engine.bootstrap_peaks(rows[[1, 3]], [[0, 1]], 64, "permutation", 50, seed=6)[0], 95)


def test_localize_with_device_bootstrap(golden, tmp_path, monkeypatch):
    """test_gpu_localize.test_calibration_correction_and_metrics with localization.bootstrap_rng = "device": the position and the
    metrics are the fixture's (weights depend on the SNR only; the fixture's pairs are significant by a wide margin)."""
    from pyaudiolocalization_amd import main as M
    monkeypatch.chdir(tmp_path)
    g = golden("localize_extras.npz")
    base, delays, gains, fs, total, trim = stages.loc_case()
    o = stages.OracleImpl()
    filt = o.prefilter(o.synchronize(o.simulate(base, delays, gains, fs, total, trim), fs), fs)
    monkeypatch.setattr(M, "simulate_signals_with_multipath", lambda **kw: [r for r in filt])
    monkeypatch.setattr(M, "synchronize_signals_improved", lambda s, fs_: s)
    monkeypatch.setattr(M, "noise_reduction_rows", lambda rows, fs_, method="butterworth": np.asarray(rows))
    cfg = cases.loc_config(True)
    cfg["localization"] = dict(cfg["localization"], bootstrap_rng="device", bootstrap_seed=17)
    state = np.random.get_state()
    full = M.localize_sound_source(cfg, calibration_data=cases.LOC_CALIBRATION, use_simulation=True, show_plots=False)
    assert np.array_equal(np.random.get_state()[1], state[1])      # the global NumPy RNG is not drawn from
    assert np.max(np.abs(full["estimated_position"] - g["loc_position_metrics"])) <= 1e-3
    metrics = full["correlation_metrics"]
    pairs = [tuple(int(v) for v in p) for p in g["loc_metric_pairs"]]
    assert sorted(metrics) == pairs
    snr = np.array([metrics[p]["snr"] for p in pairs])
    ptp = np.array([metrics[p]["peak_to_peak_ratio"] for p in pairs])
    assert np.allclose(snr, g["loc_snr"], rtol=1e-9) and np.allclose(ptp, g["loc_ptp"], rtol=1e-9)
    assert [bool(metrics[p]["significant"]) for p in pairs] == [bool(v) for v in g["loc_significant"]]


def test_invalid_input(engine):
    import ctypes as C
    from pyaudiolocalization_amd import _ffi
    rows = _frame(3, 600)
    with pytest.raises(ValueError):
        engine.bootstrap_peaks(rows, [[0, 3]], 4)
    with pytest.raises(ValueError):
        engine.bootstrap_peaks(rows, [[-1, 2]], 4)
    with pytest.raises(ValueError):
        engine.bootstrap_peaks(rows, [[0, 1]], 4, mode="jackknife")
    # the library's own checks (the Python wrapper checks mode / block_size / num_bootstrap first)
    pr = np.array([[0, 1]], dtype=np.int32)
    out = np.empty(4)
    for mode, bs, S in ((3, 50, 4), (0, 0, 4), (1, 50, 0)):
        rc = engine._lib.pal_bootstrap_peaks(engine._h, rows.ctypes.data, 3, 600, pr.ctypes.data, 1, S, mode, bs, C.c_uint64(0),
                                             out.ctypes.data)
        assert rc == _ffi.ERR_INVALID, (mode, bs, S)
    # a device pair list with a row outside the batch: reported by synchronize, never read out of range
    d_rows, d_pairs, d_peaks = engine.alloc(rows.nbytes), engine.alloc(16), engine.alloc(2 * 4 * 8)
    try:
        engine.upload(d_rows, rows)
        engine.upload(d_pairs, np.array([[0, 1], [2, 7]], dtype=np.int32))
        engine.bootstrap_peaks_dev(d_rows, 3, 600, d_pairs, 2, 4, "permutation", 50, 0, d_peaks)
        with pytest.raises(ValueError):
            engine.synchronize()
        engine.synchronize()                                       # the report is cleared
    finally:
        engine.free(d_peaks)
        engine.free(d_pairs)
        engine.free(d_rows)
