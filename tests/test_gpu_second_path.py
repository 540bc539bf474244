"""Edge shapes of the second path (csrc/sim.hip) against the oracle and against exact references: the inputs come from
tests/second_path.py, and tests/test_host_second_path.py pins the oracle itself at these shapes.

Tolerances: filtfilt is bitwise (the engine and the oracle state the same multiply-then-add recurrence and sim.hip is
built with contraction off); 1e-13 wiener3, 1e-14 compression, 1e-12 fractional_delay, 1e-11 multipath synthesis and
1e-10 correlation values are the ones the suite already uses for these operations (tests/test_gpu_parity.py,
tests/test_gpu_stream.py), scaled by the row's magnitude where the rows are not of unit scale.  Whole-sample delays
are also held to max(4 x the oracle's own error against the exact shift on the same input, 1e-14), computed from the
oracle inside the test.  Row energies: N 2^-53 fsum, the bound of any summation order.
"""
import contextlib
import warnings

import numpy as np
import pytest

from oracle import pal_oracle as O
from pyaudiolocalization_amd._ffi import PalError

import second_path as S

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _all_sentinel(x):
    return bool(np.all(_bits(x) == np.uint64(S.SENTINEL_BITS)))


@contextlib.contextmanager
def _device(engine, *hosts):
    """device copies of the host arrays (an int: that many doubles of sentinel); freed on the way out"""
    ptrs = []
    try:
        for h in hosts:
            arr = np.full(h, S.SENTINEL) if isinstance(h, int) else np.ascontiguousarray(h, dtype=np.float64)
            ptrs.append(engine.alloc(max(8, arr.nbytes)))
            if arr.nbytes:
                engine.upload(ptrs[-1], arr)
        yield ptrs
    finally:
        for p in ptrs:
            engine.free(p)


def _still_works(engine):
    """after a refusal the engine computes as before"""
    b, a = S.FILTERS["butter1"]
    assert np.array_equal(engine.filtfilt(b, a, S.zi("butter1"), S.filter_pool_row("butter1", 7, 0)), S.filter_want("butter1", 7, 0))


# ================================================================================================ filtfilt
FILT_CASES = [(name, i) for name in sorted(S.FILTERS) for i in range(5)]


@pytest.mark.parametrize("name,which", FILT_CASES, ids=["%s-%s" % (n, ("pad+1", "pad+2", "64m-1", "64m", "64m+1")[i]) for n, i in FILT_CASES])
def test_filtfilt_row_counts_and_tile_edges(engine, name, which):
    """k_filtfilt<0> at K = 2, 3, 4, 5, 101 and k_filtfilt<11>; nb != na ('fir5', 'fir101', 'short_b'), a[0] = 2.5 ('scaled');
    a second workgroup (65 and 130 rows) and partly filled wavefronts (1, 63, 65, 130 rows); rows one and two samples longer
    than the pad length; extended lengths on either side of a 64-sample tile edge.  Bitwise against O.filtfilt."""
    b, a = S.FILTERS[name]
    zi = S.zi(name)
    n = S.gpu_lengths(name)[which]
    assert n > 3 * S.taps(name)
    for r in S.filter_rows(name):
        idx = S.filter_batch_indices(r)
        rows = np.array([S.filter_pool_row(name, n, i) for i in idx])
        want = np.array([S.filter_want(name, n, i) for i in idx])
        got = engine.filtfilt(b, a, zi, rows)
        for q in range(r):
            assert np.array_equal(got[q], want[q]), (name, n, r, q, float(np.max(np.abs(got[q] - want[q]))))
        # the device-resident form writes exactly R N doubles
        with _device(engine, rows, r * n + 64) as (d_in, d_out):
            engine.filtfilt_dev(b, a, zi, d_in, r, n, d_out)
            engine.synchronize()
            back = engine.download(np.empty(r * n + 64), d_out)
        assert _same_bits(back[: r * n].reshape(r, n), got), (name, n, r)
        assert _all_sentinel(back[r * n:]), (name, n, r)
        # a row of a batch equals the same row filtered alone
        for q in sorted({0, r // 2, min(r - 1, 62), min(r - 1, 63), min(r - 1, 64), r - 1}):
            assert _same_bits(engine.filtfilt(b, a, zi, rows[q]), got[q]), (name, n, r, q)
    for special in (S.CONSTANT_ROW, S.STEP_ROW):                     # (a batch of one row holds neither)
        assert np.array_equal(engine.filtfilt(b, a, zi, S.filter_pool_row(name, n, special)), S.filter_want(name, n, special))


@pytest.mark.parametrize("name", ["butter5bp", "butter3"])
def test_filtfilt_ragged_lengths_offsets_and_stray_stores(engine, name):
    """70 rows of lengths 3K+1 .. 3K+400 in one launch: backward tiles of unequal length, the second workgroup partly
    filled and holding the longest row; gaps between the rows, a permuted output order and the tail keep the sentinel."""
    b, a = S.FILTERS[name]
    lengths, in_off, out_off, in_buf, out_len, rows = S.ragged_case(name)
    with _device(engine, in_buf, out_len) as (d_in, d_out):
        engine.filtfilt_ragged_dev(b, a, S.zi(name), d_in, d_out, in_off, out_off, lengths)
        engine.synchronize()
        out = engine.download(np.empty(out_len), d_out)
        back = engine.download(np.empty(in_buf.shape[0]), d_in)
    assert _same_bits(back, in_buf)                                  # the input is read only
    written = np.zeros(out_len, dtype=bool)
    for r in range(S.RAGGED_R):
        got = out[out_off[r]: out_off[r] + lengths[r]]
        want = O.filtfilt(b, a, rows[r])
        assert np.array_equal(got, want), (name, r, int(lengths[r]), float(np.max(np.abs(got - want))))
        written[out_off[r]: out_off[r] + lengths[r]] = True
    assert int(written.sum()) == int(lengths.sum())                  # (the rows do not overlap)
    assert _all_sentinel(out[~written]) and int((~written).sum()) >= 64 + S.RAGGED_R


def test_filtfilt_refusals(engine):
    b, a = S.FILTERS["butter3"]
    zi, k = S.zi("butter3"), S.taps("butter3")
    with pytest.raises(ValueError, match="padlen, which is %d" % (3 * k)):
        engine.filtfilt(b, a, zi, np.ones((2, 3 * k)))
    _still_works(engine)
    with pytest.raises(PalError):
        engine.filtfilt([1.0], [1.0], [0.0], np.ones(50))            # K = 1: no recurrence state
    _still_works(engine)
    with pytest.raises(PalError):
        engine.filtfilt(np.ones(513) / 513, [1.0], np.zeros(512), np.ones(2000))
    _still_works(engine)
    with pytest.raises(ValueError):
        engine.filtfilt(b, np.concatenate(([0.0], a[1:])), zi, np.ones(100))
    _still_works(engine)
    n = 3 * k + 5
    with _device(engine, np.ones(3 * n), 3 * n) as (d_in, d_out):
        with pytest.raises(ValueError, match="padlen"):
            engine.filtfilt_ragged_dev(b, a, zi, d_in, d_out, [0, n, 2 * n], [0, n, 2 * n], [n, 3 * k, n])
        with pytest.raises(ValueError):
            engine.filtfilt_ragged_dev(b, a, zi, d_in, d_out, [0, -1, 2 * n], [0, n, 2 * n], [n, n, n])
        with pytest.raises(ValueError):
            engine.filtfilt_ragged_dev(b, a, zi, d_in, d_out, [0, n, 2 * n], [0, n, -8], [n, n, n])
        engine.synchronize()
        assert _all_sentinel(engine.download(np.empty(3 * n), d_out))   # a refused call writes nothing
    _still_works(engine)


# ================================================================================================ wiener3
WIENER_MIXES = (("normal", "zeros", "spike"), ("constant", "tiny", "huge"), ("step", "ints", "normal"))


def _check_wiener(got, row, tag):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want = O.wiener3(row)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    ok = ~np.isnan(want)
    if ok.any():
        tol = 1e-13 * max(1.0, float(np.max(np.abs(row))))
        assert float(np.max(np.abs(got[ok] - want[ok]))) <= tol, (tag, float(np.max(np.abs(got[ok] - want[ok]))), tol)
    return want


@pytest.mark.parametrize("n", (1, 2, 3, 255, 256, 257, 1000))
def test_wiener3_families_and_row_stride(engine, n):
    """N below, at and past the 256-lane workgroup; one batch per family, and batches of three different families (the
    noise estimate is per row); NaN exactly where numpy has NaN."""
    for fam in S.FAMILIES:
        row = S.family(fam, [50, n], n)
        want = _check_wiener(engine.wiener3(row), row, (fam, n))
        if fam == "zeros":
            assert np.all(np.isnan(want))                            # 0 / 0, as scipy
    # squares that underflow to zero: all-NaN like numpy's ('tiny' itself, 1e-160, still has subnormal squares and stays finite)
    row = S.family("tiny", [50, n], n) * 1e-10
    want = _check_wiener(engine.wiener3(row), row, ("underflow", n))
    assert np.all(np.isnan(want))
    for mix in WIENER_MIXES:
        rows = np.array([S.family(fam, [51, n, q], n) for q, fam in enumerate(mix)])
        got = engine.wiener3(rows)
        for q, fam in enumerate(mix):
            _check_wiener(got[q], rows[q], (mix, fam, n))
            assert _same_bits(engine.wiener3(rows[q]), got[q]), (mix, fam, n)
        with _device(engine, rows, 3 * n + 64) as (d_in, d_out):
            engine.wiener3_dev(d_in, 3, n, d_out)
            engine.synchronize()
            back = engine.download(np.empty(3 * n + 64), d_out)
        assert _same_bits(back[: 3 * n].reshape(3, n), got) and _all_sentinel(back[3 * n:])


# ================================================================================================ normalize / compress
def _norm_rows(n):
    rng = np.random.default_rng([60, n])
    rows = np.zeros((4, n))
    rows[0] = rng.standard_normal(n) * 1e3                           # (row 1 stays zero between live rows)
    rows[2] = rng.uniform(-0.5, 0.5, n) * 1e-5
    rows[2, n - 1] = -1e-5                                           # the maximum: last sample, negative
    rows[3] = rng.integers(-1, 2, n) * 5e-324                        # denormals only
    rows[3, n // 2] = 5e-324
    return rows


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_normalize_compress_rows(engine, n):
    rows = _norm_rows(n)
    assert float(np.max(np.abs(rows[3]))) == 5e-324 and not rows[1].any()
    live = (0, 2, 3)
    top = {q: int(np.argmax(np.abs(rows[q]))) for q in live}
    assert top[2] == n - 1 and rows[2, n - 1] < 0
    got = engine.normalize_compress(rows, normalize_only=True)
    for q in range(4):
        assert np.array_equal(got[q], O.normalize_signal(rows[q])), (n, q)
    for q in live:
        assert got[q, top[q]] == np.sign(rows[q, top[q]])
    assert _same_bits(got[1], np.zeros(n))
    for thr, eps in ((0.8, 1e-8), (0.25, 1e-3)):
        got = engine.normalize_compress(rows, threshold=thr, epsilon=eps)
        for q in range(4):
            want = O.dynamic_range_compression(rows[q], thr, eps)
            assert float(np.max(np.abs(got[q] - want))) <= 1e-14, (n, q, thr)
            assert _same_bits(engine.normalize_compress(rows[q], threshold=thr, epsilon=eps), got[q])
        for q in live:
            assert got[q, top[q]] == np.sign(rows[q, top[q]]), (n, q, thr)      # exactly +-1: the one-reduction shortcut
        assert not got[1].any()


# ================================================================================================ fractional_delay
FD_DELAYS = np.array([0.0, 1.0, 7.0, 0.37, 12.5]) / S.FS


@pytest.mark.parametrize("n", (100, 101, 199, 200, 299, 300, 1024, 1501))
def test_fractional_delay_fade_lengths(engine, n):
    """int(0.01 N) = 1 (N = 100 .. 199), 2 (200 .. 299) and 3 or more: SimStorer::fade's special cases and the general ramp"""
    rows = np.array([S.family("normal", [70, n, q], n) for q in range(5)])
    got = engine.fractional_delay(rows, FD_DELAYS, S.FS)
    for q in range(5):
        want = O.fractional_delay(rows[q], FD_DELAYS[q], S.FS)
        assert float(np.max(np.abs(got[q] - want))) <= 1e-12, (n, q, float(np.max(np.abs(got[q] - want))))
        # (not bitwise: two rows share one complex transform, so a row's rounding depends on its partner)
        alone = engine.fractional_delay(rows[q], FD_DELAYS[q], S.FS)
        assert float(np.max(np.abs(alone - want))) <= 1e-12, (n, q, float(np.max(np.abs(alone - want))))
    for q, k in ((0, 0), (1, 1), (2, 7)):
        exact = S.exact_shift(rows[q], k)
        own = float(np.max(np.abs(O.fractional_delay(rows[q], FD_DELAYS[q], S.FS) - exact)))
        bound = max(4 * own, 1e-14)
        err = float(np.max(np.abs(got[q] - exact)))
        print("fractional_delay N=%d k=%d: engine - exact %.3g, oracle - exact %.3g" % (n, k, err, own))
        assert err <= bound, (n, k, err, bound)
    assert not got[:, 0].any()                                       # +-0.0
    if int(0.01 * n) >= 2:
        assert not got[:, n - 1].any()
    else:
        assert np.all(got[:, n - 1] != 0)                            # a fade of one sample leaves the last one alone


def test_fractional_delay_refusals(engine):
    with pytest.raises(ValueError):
        engine.fractional_delay(np.ones(99), 0.001, S.FS)
    _still_works(engine)
    with pytest.raises(PalError):
        engine.fractional_delay(np.ones((1, 2 ** 19 + 1)), [0.001], S.FS)
    _still_works(engine)


# ================================================================================================ simulate_multipath
SIM_B, SIM_M, SIM_NBASE, SIM_TOTAL = 3, 5, 1500, 1700
SIM_SILENT = (0, 2)                                                  # flat row 2: packed with the live row 3


def _sim_tables(k):
    rng = np.random.default_rng([80, k])
    base = rng.standard_normal((SIM_B, SIM_NBASE))
    delays = rng.uniform(0.0, 0.02, (SIM_B, SIM_M, k))
    gains = rng.choice([-1.0, 1.0], (SIM_B, SIM_M, k)) * 10.0 ** rng.uniform(-3.0, 0.0, (SIM_B, SIM_M, k))
    gains[SIM_SILENT] = 0.0
    return base, delays, gains


@pytest.mark.parametrize("k", (1, 7))
def test_simulate_multipath_trims_groups_and_silent_microphone(engine, k):
    base, delays, gains = _sim_tables(k)
    for trim in (0, 1500, 1700, 2000):
        out_len = trim if 0 < trim < SIM_TOTAL else SIM_TOTAL
        got = engine.simulate_multipath(base, S.FS, SIM_TOTAL, delays, gains, trim)
        assert got.shape == (SIM_B, SIM_M, out_len)
        for f in range(SIM_B):
            want = O.simulate_from_base(base[f], delays[f], gains[f], S.FS, SIM_TOTAL, trim if trim > 0 else None)
            assert want.shape == (SIM_M, out_len)
            assert float(np.max(np.abs(got[f] - want))) <= 1e-11, (k, trim, f, float(np.max(np.abs(got[f] - want))))
        assert not got[SIM_SILENT].any()                             # exactly zero, as the reference's sum of 0 * delayed rows
        assert np.all(np.max(np.abs(got.reshape(SIM_B * SIM_M, -1)), axis=1)[np.arange(SIM_B * SIM_M) != 2] == 1.0)
        try:
            engine.set_chunk(2)                                      # 15 rows = 8 packed transforms: four launch groups
            again = engine.simulate_multipath(base, S.FS, SIM_TOTAL, delays, gains, trim)
        finally:
            engine.set_chunk(0)
        assert again.tobytes() == got.tobytes(), (k, trim)
        with _device(engine, base, delays, gains, SIM_B * SIM_M * out_len + 64) as (d_base, d_delays, d_gains, d_out):
            engine.simulate_multipath_dev(d_base, SIM_B, SIM_NBASE, S.FS, SIM_TOTAL, d_delays, d_gains, SIM_M, k, trim, d_out)
            engine.synchronize()
            back = engine.download(np.empty(SIM_B * SIM_M * out_len + 64), d_out)
            kept = engine.download(np.empty(gains.size), d_gains)
        assert back[: got.size].tobytes() == got.tobytes() and _all_sentinel(back[got.size:]), (k, trim)
        assert _same_bits(kept, gains.ravel())                       # the caller's gain table is not rescaled in place


def test_simulate_multipath_refusals(engine):
    base, delays, gains = _sim_tables(1)
    with pytest.raises(ValueError):
        engine.simulate_multipath(base, S.FS, SIM_NBASE - 1, delays, gains)        # nbase > total_samples
    _still_works(engine)
    with pytest.raises(ValueError):
        engine.simulate_multipath(base[:, :90], S.FS, 99, delays, gains)
    _still_works(engine)


# ================================================================================================ xcorr / sync / energies
@pytest.mark.parametrize("n", S.XCORR_N)
def test_xcorr_vs_ref_integer_rows(engine, n):
    """N from one sample (a correlation of one point, four NaN slots) to past a power of two; R = 1, 2, 7; the reference row
    first, in the middle and last; against np.correlate, which is exact on these rows."""
    for r in S.XCORR_R:
        case = S.xcorr_case(n, r)
        for ref in case.refs:
            measured = engine.xcorr_vs_ref(case.rows, ref)
            S.check_xcorr(measured, case.exact[ref], ref, n, (case.name, ref))
            if r == 7:
                try:
                    engine.set_chunk(2)                              # 4 packed transforms: two launch groups, the second with row0 = 4
                    again = engine.xcorr_vs_ref(case.rows, ref)
                finally:
                    engine.set_chunk(0)
                for x, y in zip(measured[:3], again[:3]):
                    assert x.tobytes() == y.tobytes(), (case.name, ref)
                assert measured[3] == again[3]
                try:
                    engine.set_chunk(1)                              # four groups, the last with a single row
                    again = engine.xcorr_vs_ref(case.rows, ref)
                finally:
                    engine.set_chunk(0)
                for x, y in zip(measured[:3], again[:3]):
                    assert x.tobytes() == y.tobytes(), (case.name, ref)


@pytest.mark.parametrize("n", (5, 64))
def test_xcorr_crafted_peaks_and_synchronize(engine, n):
    """peaks at index 0, 1, 2, N-1, 2N-4, 2N-3 and 2N-2: the NaN slots of win5, and the host code that must not read them"""
    from pyaudiolocalization_amd.utils import synchronize_signals_improved
    for case in S.crafted_cases(n):
        ref = case.refs[0]
        kpk, win, pk, refpk = engine.xcorr_vs_ref(case.rows, ref)
        S.check_xcorr((kpk, win, pk, refpk), case.exact[ref], ref, n, case.name)
        assert refpk == 16.0
        neg = 3 if "low" in case.name else 4
        assert win[neg, 2] < 0 < pk[neg] and pk[neg] == -win[neg, 2]
        if "low" in case.name:
            assert kpk.tolist()[:3] == [0, 1, 2]
            assert np.isnan(win[0]).tolist() == [True, True, False, False, False]
            assert np.isnan(win[1]).tolist() == [True, False, False, False, False]
            assert not np.isnan(win[2]).any()
        else:
            assert kpk.tolist()[1:4] == [2 * n - 4, 2 * n - 3, 2 * n - 2]
            assert not np.isnan(win[1]).any()
            assert np.isnan(win[2]).tolist() == [False, False, False, False, True]
            assert np.isnan(win[3]).tolist() == [False, False, False, True, True]
        got = synchronize_signals_improved(list(case.rows), S.FS)
        want = O.synchronize_signals(list(case.rows), S.FS)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), case.name


def test_sync_measure_dev_odd_microphone_count(engine):
    """M = 5: the int32 result block of frame b starts at an odd offset; every frame's block is that frame's xcorr_vs_ref"""
    frames, refs, exact = S.sync_case()
    with _device(engine, frames) as (d_rows,):
        ref, kpk, win, pk, refpk = engine.sync_measure_dev(d_rows, S.SYNC_B, S.SYNC_M, S.SYNC_N)
    assert ref.tolist() == refs
    for f in range(S.SYNC_B):
        S.check_xcorr((kpk[f], win[f], pk[f], refpk[f]), exact[f], refs[f], S.SYNC_N, ("sync", f))
        alone = engine.xcorr_vs_ref(frames[f], refs[f])
        assert kpk[f].tobytes() == alone[0].tobytes() and win[f].tobytes() == alone[1].tobytes()
        assert pk[f].tobytes() == alone[2].tobytes() and refpk[f] == alone[3]


@pytest.mark.parametrize("n", (1, 255, 256, 257, 6000))
def test_row_energies_dev(engine, n):
    fams = ("normal", "zeros", "ints", "normal", "ints")
    rows = np.array([S.family(fam, [90, n, q], n) for q, fam in enumerate(fams)])
    with _device(engine, rows) as (d_rows,):
        got = engine.row_energies_dev(d_rows, len(fams), n)
    for q, fam in enumerate(fams):
        want = S.fsum_energy(rows[q])
        if fam == "normal":
            assert abs(got[q] - want) <= n * 2.0 ** -53 * want, (n, q, got[q], want)
        else:
            assert got[q] == want, (n, q, fam)


# ================================================================================================ align_rows
@pytest.mark.parametrize("lout", (1000, 1001, 17421))
def test_align_rows_dev(engine, lout):
    """Lout = 17421 is past 64 x 256: the grid-stride loop of k_align_rows wraps"""
    r, n = 5, 1000
    rows = np.array([S.family("normal", [95, q], n) for q in range(r)])
    valid = [p for p in (0, 1, 255, 256, lout - n) if p <= lout - n]
    pads = [p if p <= lout - n else valid[q % len(valid)] for q, p in enumerate((0, 1, 255, 256, lout - n))]
    with _device(engine, rows, r * lout + 64) as (d_rows, d_out):
        engine.align_rows_dev(d_rows, r, n, pads, lout, d_out)
        engine.synchronize()
        back = engine.download(np.empty(r * lout + 64), d_out)
        for bad_pads, bad_lout in (([0, -1, 0, 0, 0], lout), ([0, 0, lout - n + 1, 0, 0], lout), ([0] * r, n - 1)):
            with pytest.raises(ValueError):
                engine.align_rows_dev(d_rows, r, n, bad_pads, bad_lout, d_out)
        engine.synchronize()
        assert _same_bits(engine.download(np.empty(r * lout + 64), d_out), back)    # a refused call writes nothing
    want = np.array([np.pad(rows[q], (pads[q], lout - n - pads[q])) for q in range(r)])
    assert np.array_equal(back[: r * lout].reshape(r, lout), want)
    assert _all_sentinel(back[r * lout:])
    _still_works(engine)
