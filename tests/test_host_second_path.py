"""The oracle's standing at the edge shapes of the second path (no GPU): ``oracle/pal_oracle.py`` against scipy and
against exact references, at the shapes where tests/test_gpu_second_path.py then holds the HIP kernels to the oracle.

Measured here (scipy 1.15.3, NumPy's pocketfft):

* ``O.filtfilt`` is bit-identical to ``scipy.signal.filtfilt`` for every filter of ``second_path.FILTERS`` at
  N = 3K+1, 3K+2, 3K+63, 3K+64, 6K+130, except ``fir101`` (within 1.2e-15; bound 1e-13, the project's FIR tolerance).
* ``O.wiener3`` is bit-identical to ``scipy.signal.wiener``, NaN pattern included.  All-zero rows are all-NaN in both
  (0 / 0 in ``1 - noise / var``).  'tiny' rows (normal x 1e-160) are NOT: their squares are subnormal (1e-320), not zero,
  and both return finite values; only below about 1e-162 do the squares underflow and both turn all-NaN.
* ``O.xcorr_full`` against ``np.correlate`` on integer rows (exact): within 5e-13 for N <= 1025.
* ``O.fractional_delay`` against the exact shifted row times the fade window, max |error| over 'normal' rows:

      N      k = 0     k = 1     k = 7
      100    5.0e-16   8.9e-16   2.0e-15
      199    1.8e-15   1.8e-15   5.4e-15
      200    8.9e-16   8.9e-16   2.1e-15
      299    8.9e-16   7.8e-16   2.2e-15
      300    8.9e-16   6.7e-16   2.5e-15
      1501   1.3e-15   1.3e-15   3.8e-15

  This is the reference's own error: the GPU test allows the engine four times the oracle's error on the same input
  (floor 1e-14).  The bound asserted here is the textbook one for a transform pair, 8 u log2(2N) max|x| with
  u = 2^-53 (4 u log2 n per transform, Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2).
"""
import math
import warnings

import numpy as np
import pytest

import scipy.signal as scipy_signal

from oracle import pal_oracle as O

import second_path as S


@pytest.mark.parametrize("name", sorted(S.FILTERS))
def test_oracle_filtfilt_is_scipys(name):
    b, a = S.FILTERS[name]
    for n in S.host_lengths(name):
        for fam in ("normal", "constant", "step"):
            x = S.family(fam, [40, n], n)
            got, want = O.filtfilt(b, a, x), scipy_signal.filtfilt(b, a, x)
            if name == "fir101":
                assert np.max(np.abs(got - want)) <= 1e-13, (n, fam)
            else:
                assert np.array_equal(got, want), (n, fam, float(np.max(np.abs(got - want))))
    n = 3 * S.taps(name)
    with pytest.raises(ValueError, match="padlen"):
        O.filtfilt(b, a, np.ones(n))
    with pytest.raises(ValueError, match="padlen"):
        scipy_signal.filtfilt(b, a, np.ones(n))


@pytest.mark.parametrize("fam", [f for f in S.FAMILIES if f not in ("tiny", "huge")])
def test_oracle_wiener3_is_scipys(fam):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                              # 0 / 0 of the all-zero rows, in both
        for n in (1, 2, 3, 257):
            x = S.family(fam, [41, n], n)
            got, want = O.wiener3(x), scipy_signal.wiener(x)
            assert np.array_equal(got, want, equal_nan=True), (fam, n)
            if fam == "zeros":
                assert np.all(np.isnan(got))


def test_wiener3_underflow_rows_are_nan_in_numpy_too():
    """squares that underflow to zero leave noise = var = 0: all-NaN, as an all-zero row; 1e-160 does not underflow yet"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for n in (3, 257):
            x = S.family("tiny", [41, n], n)
            assert np.all(np.isfinite(scipy_signal.wiener(x))) and np.all(np.isfinite(O.wiener3(x)))
            assert np.all(np.isnan(scipy_signal.wiener(x * 1e-10))) and np.all(np.isnan(O.wiener3(x * 1e-10)))


def test_correlation_inputs_have_unique_peaks():
    assert S.all_xcorr_inputs() > 200                                # every builder assertion ran, over this many rows


@pytest.mark.parametrize("n", S.XCORR_N)
def test_oracle_xcorr_against_exact(n):
    for r in S.XCORR_R:
        case = S.xcorr_case(n, r)
        for ref in case.refs:
            for q, row in enumerate(case.rows):
                exact = case.exact[ref][q]
                got = O.xcorr_full(row, case.rows[ref])
                assert got.shape == exact.shape == (2 * n - 1,)
                assert np.max(np.abs(got - exact)) <= 1e-10 * max(1.0, float(np.max(np.abs(exact))))
    if n >= 5:
        for case in S.crafted_cases(min(n, 64)):
            ref = case.refs[0]
            for q, row in enumerate(case.rows):
                assert np.max(np.abs(O.xcorr_full(row, case.rows[ref]) - case.exact[ref][q])) <= 1e-10 * 16.0


@pytest.mark.parametrize("n", (100, 199, 200, 299, 300, 1501))
def test_oracle_fractional_delay_against_exact_shift(n):
    assert S.exact_shift(np.arange(1.0, n + 1.0), 0)[0] == 0.0       # the fade starts at 0 for every fade length, 1 included
    for k in (0, 1, 7):
        x = S.family("normal", [42, n, k], n)
        err = float(np.max(np.abs(O.fractional_delay(x, k / S.FS, S.FS) - S.exact_shift(x, k))))
        bound = 8 * 2.0 ** -53 * math.log2(2 * n) * float(np.max(np.abs(x)))
        print("fractional_delay N=%d k=%d: oracle - exact = %.3g (bound %.3g)" % (n, k, err, bound))
        assert err <= bound, (n, k, err, bound)


def test_fade_window_special_lengths():
    """int(0.01 N) = 1 fades only sample 0 (np.linspace(1, 0, 1) is [1.]); 2 zeroes both end samples"""
    w = O.fade_window(199)
    assert w[0] == 0.0 and np.all(w[1:] == 1.0)
    w = O.fade_window(200)
    assert w[0] == 0.0 and w[-1] == 0.0 and np.all(w[1:-1] == 1.0)
    w = O.fade_window(300)
    assert w[:3].tolist() == [0.0, 0.5, 1.0] and w[-3:].tolist() == [1.0, 0.5, 0.0]
