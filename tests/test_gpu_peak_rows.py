"""Peak selection (csrc/peaks.hip) on crafted correlation rows: Engine.select_peaks against the oracle, row by row, on every
entry of tests/peak_rows.py.  Integers and copied row values are compared for equality on every row of every entry - none is
skipped and none is excused by a tolerance; only the SNR, a quotient of floating sums, has a bound (1e-9, the suite's)."""
import warnings

import numpy as np
import pytest

from oracle import pal_oracle as O

import peak_rows as P

pytestmark = pytest.mark.gpu

SNR_RTOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _engine(engine):
    """The drop-in modules use the process-wide default engine; make it the session engine."""
    import pyaudiolocalization_amd.engine as E
    E._default = engine
    yield
    E._default = None


def check_entry(engine, e):
    table, ks = engine.select_peaks(e.rows, e.n2, e.fs, e.num_peaks, e.method, e.mult, e.med)
    want = P.expected(e)
    assert table.shape == (len(want),) and ks.shape == (len(want), e.num_peaks)
    for field in ("n_sel", "branch", "k_sel", "k_argmax"):
        exp = np.array([w[field] for w in want])
        bad = np.flatnonzero(table[field] != exp)
        assert bad.size == 0, (e.name, field, bad[:8], table[field][bad[:8]], exp[bad[:8]])
    for r, w in enumerate(want):
        m = w["n_sel"]
        assert np.array_equal(ks[r, :m], w["k"]), (e.name, r, ks[r, :m][:8], w["k"][:8])
        assert np.all(ks[r, m:] == -1), (e.name, r)
    for field in ("cmax", "cmin", "sel_height"):                  # copies of row values: equal, not close
        exp = np.array([w[field] for w in want])
        assert np.array_equal(table[field], exp), (e.name, field)
    check_snr(table["snr"], np.array([w["snr"] for w in want]), SNR_RTOL, e.name)


def check_snr(got, exp, rtol, what):
    """inf matches inf, NaN (n = 1, 2: no noise region) matches NaN, everything else to rtol"""
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(np.isfinite(exp) & (exp != 0), np.abs(got - exp) / np.abs(exp), 0.0)
    print(what, "snr: largest relative difference %.3g" % np.nanmax(rel, initial=0.0))
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=0, equal_nan=True, err_msg=what)


@pytest.mark.parametrize("family", P.FAMILIES)
def test_corpus_family(engine, family):
    entries = list(P.corpus(family))
    assert entries
    for e in entries:
        check_entry(engine, e)


def metric_rows():
    rows = [("offset c/sigma=%g" % c, row) for c, row in zip(P.OFFSETS, P.offset_rows())]
    rows += [(e.name + " row 0", e.rows[0]) for e in P.corpus("tiny") if e.name.endswith("_median")]
    rows += [("no_peaks row %d" % r, row) for r, row in enumerate(next(P.corpus("no_peaks")).rows)]
    return rows


def test_metrics_entry_and_dropins(engine):
    """pal_corr_metrics (Engine.corr_metrics) and the two public drop-ins that sit on it, on the offset, tiny and no-peak rows."""
    from pyaudiolocalization_amd import utils
    got_snr, exp_snr = [], []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                                           # np.std of an empty noise region (n = 1, 2)
        for what, row in metric_rows():
            rec = engine.corr_metrics(row)
            assert int(rec["k_argmax"]) == int(np.argmax(row)), what
            assert float(rec["cmax"]) == float(np.max(row)) and float(rec["cmin"]) == float(np.min(row)), what
            got_snr.append(float(rec["snr"]))
            exp_snr.append(float(O.compute_snr(row)))
            assert np.array_equal(utils.compute_snr(row), got_snr[-1], equal_nan=True), what   # the drop-in is the same call
            ratio, exp_ratio = utils.compute_peak_to_peak_ratio(row), O.compute_peak_to_peak_ratio(row)
            assert ratio == exp_ratio, (what, ratio, exp_ratio)                   # a quotient of two copied values: equal
    check_snr(np.array(got_snr), np.array(exp_snr), SNR_RTOL, "corr_metrics")


def test_batch_independence(engine):
    """Every row of the mixed batch (a constant row, two staircases, a plateau row and noise rows side by side) alone gives what it gave
    in the batch: integers equal; the SNR to 1e-11, since a row sent alone is cut into other segments and summed in another order."""
    for e in P.corpus("mixed"):
        table, ks = engine.select_peaks(e.rows, e.n2, e.fs, e.num_peaks, e.method, e.mult, e.med)
        for r, row in enumerate(e.rows):
            one, k1 = engine.select_peaks(row, e.n2, e.fs, e.num_peaks, e.method, e.mult, e.med)
            for field in ("n_sel", "branch", "k_sel", "k_argmax", "cmax", "cmin", "sel_height"):
                assert one[field][0] == table[field][r], (e.name, r, field)
            assert np.array_equal(k1[0], ks[r]), (e.name, r)
            np.testing.assert_allclose(one["snr"][0], table["snr"][r], rtol=1e-11, atol=0)


def test_cross_route(engine):
    """select_peaks on the correlation a get_time_delays_phat call returned reproduces that call's own selection and record."""
    rng = np.random.default_rng(7)
    for n, fs, npk, method, med in ((3000, 48000.0, 3, "median", None), (4097, 8000.0, 5, "adaptive", 0.01), (12000, 44100.0, 1, "median", 0.002)):
        a = rng.standard_normal(n)
        b = np.roll(a, int(rng.integers(-20, 20))) + 0.5 * rng.standard_normal(n)
        ks, rec, corr = engine.get_time_delays_phat(a, b, fs, npk, method, 1.0, med)
        table, k2 = engine.select_peaks(corr, n, fs, npk, method, 1.0, med)
        m = int(rec["n_sel"])
        assert np.array_equal(k2[0, :m], ks) and np.all(k2[0, m:] == -1)
        for field in ("n_sel", "branch", "k_sel", "k_argmax", "cmax", "cmin", "sel_height"):
            assert table[field][0] == rec[field], field
        np.testing.assert_allclose(table["snr"][0], rec["snr"], rtol=SNR_RTOL, atol=0)


def test_argument_errors(engine):
    x = np.random.default_rng(1).standard_normal((2, 64))
    with pytest.raises(ValueError):
        engine.select_peaks(np.zeros((0, 64)), 32, 8000.0)             # R = 0
    with pytest.raises(ValueError):
        engine.select_peaks(x, 0, 8000.0)                              # n2 = 0
    with pytest.raises(ValueError):
        engine.select_peaks(x, 65, 8000.0)                             # n2 > n
    with pytest.raises(ValueError):
        engine.select_peaks(x, 32, 8000.0, num_peaks=257)
    with pytest.raises(ValueError):
        engine.select_peaks(x, 32, 500.0)                              # peak_distance = int(fs * 0.001) = 0
    for bad in (np.nan, np.inf, -np.inf):                              # rejected on the host, before any launch
        y = x.copy()
        y[1, 63] = bad
        with pytest.raises(ValueError, match="non-finite"):
            engine.select_peaks(y, 32, 8000.0)
    table, ks = engine.select_peaks(x, 32, 8000.0)                     # the engine is still good
    assert table["n_sel"].min() >= 1
