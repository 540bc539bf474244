"""Conditions on the inputs of tests/test_gpu_long_frames.py, checked without a GPU (the inputs come from tests/long_frames.py):
the rows called exact are exact, the sparse correlation is np.correlate's, and every noise row is decided."""
import numpy as np
import pytest

from oracle import pal_oracle as O

import long_frames as LF
import peak_positions as PP
import second_path as S


@pytest.mark.parametrize("length", (98305, 524289))
def test_impulse_rows_are_what_the_oracle_computes(length):
    """a_i a_j / (|a_i a_j| + 1e-10) at (p_i - p_j) mod n and 0 elsewhere, within 1e-15 of O.phat_correlation (whose own
    rounding is 3.4e-16 at the peak and 1.8e-16 off it at these lengths)"""
    n = 2 * length - 1
    for f in LF.impulse_frames(length):
        if length > 100000 and f.name not in ("wrap", "tile"):         # (the oracle's transforms are the cost: 1.5 s a row there)
            continue
        for i, j, index, value in f.peaks:
            want = O.phat_correlation(f.frame[i], f.frame[j])
            assert want.shape == (n,) and 0 <= index < n
            assert np.max(np.abs(want - LF.impulse_row(length, index, value))) <= 1e-15, (length, f.name, i, j)
            assert abs(value) <= 1.0


def test_impulse_frames_reach_the_designed_indices():
    for length in LF.IMPULSE_LENGTHS:
        n = 2 * length - 1
        inv, _ = LF.geometry(length)
        assert 4 * length - 3 <= (inv.m1 << inv.l2)
        found = {p[2] for f in LF.impulse_frames(length) for p in f.peaks}
        assert {0, n - 1, length - 1, (1 << inv.l2) - 1, 1 << inv.l2, 4095, 4096} <= found, length
        signs = {np.sign(p[3]) for f in LF.impulse_frames(length) for p in f.peaks}
        assert signs == {-1.0, 1.0}
    for top in LF.TOPS:                                                # the tightest fit: three points short of the convolution
        inv, _ = LF.geometry(top)
        assert (inv.m1 << inv.l2) - (4 * top - 3) == 3, top


def test_sparse_exact_correlation_is_numpy_correlate():
    n = 700
    pos, val = LF.sparse_rows(n, LF.SPARSE_SEEDS[n])
    rows = LF.dense(pos, val, n)
    assert np.count_nonzero(rows) == 3 * LF.SPARSE_NONZERO and np.all(rows[:, 0] != 0) and np.all(rows[:, n - 1] != 0)
    assert np.max(np.abs(rows)) <= 8 and np.array_equal(rows, np.rint(rows))
    for q in range(3):
        got = LF.sparse_exact(pos[q], val[q], pos[LF.SPARSE_REF], val[LF.SPARSE_REF], n)
        assert np.array_equal(got.astype(np.float64), S.exact_xcorr(rows[q], rows[LF.SPARSE_REF])), q
    case = LF.sparse_case(n)
    assert case.refs == (LF.SPARSE_REF,) and len(case.exact[LF.SPARSE_REF]) == 3


@pytest.mark.parametrize("n", LF.SPARSE_N)
def test_sparse_rows_have_unique_peaks(n):
    """sparse_case() asserts peak_margin >= 1 and the designed peak index for every row; the committed seed is the first that passes"""
    case = LF.sparse_case(n)
    assert case.rows.shape == (3, n) and np.count_nonzero(case.rows) == 3 * LF.SPARSE_NONZERO
    assert LF.SPARSE_SEEDS[n] == 0 or LF.find_sparse_seed(n) == LF.SPARSE_SEEDS[n]


@pytest.mark.parametrize("length", LF.NOISE_LENGTHS)
def test_every_noise_row_is_decided(length):
    """The integer fields of the oracle's record do not move when its row is perturbed by 1e-11 max|corr|, two draws; all three
    rows, every window setting of the length; unwindowed, the common component is the maximum."""
    assert PP.PERTURB == 1e-11
    case = LF.noise_case(length)
    n = 2 * length - 1
    for med in LF.noise_windows(length):
        for p in range(3):
            assert PP.decided(case.corr[p], length, LF.FS, "median", 1.0, med, case.records[med][p]), (length, med, p)
    if length == LF.NOISE_LENGTHS[0]:                                  # the case's rows and records are O.phat_correlation's and O.all_pairs'
        table = O.all_pairs(case.frame, LF.FS)
        for p, (i, j) in enumerate(LF.PAIRS3):
            assert np.array_equal(case.corr[p], O.phat_correlation(case.frame[i], case.frame[j])), p
            assert all(table[key][p] == case.records[None][p][key] for key in table), p
    for p, want in enumerate(((-37) % n, 1234, 1271)):
        assert int(np.argmax(case.corr[p])) == want, (length, p)
        top = np.sort(case.corr[p])[-2:]
        assert top[1] > (0.15 if p == 2 else 0.3) and top[0] < 0.05, (length, p, top)   # (1, 2): both rows carry 0.6 of it


@pytest.mark.parametrize("length", sorted(LF.CUTS))
def test_cut_rows_sit_on_the_grid_corners_and_are_decided(length):
    """The designed rows of a cut have their maximum on CRT(r1, r2) for the first, middle and last column class and the first and
    last tile point (cut_case() asserts the oracle's argmax), and their records are decided under both threshold methods."""
    n1, n2, lm, nch = LF.CUTS[length]
    assert n1 * n2 == 2 * length - 1 and (1 << lm) >= 2 * n2 - 1 > (1 << (lm - 1)) and nch == ((n1 - 1) // 2 + 10) // 11
    ks = LF.cut_indices(length)
    assert len(ks) == 6 and {(k % n1, k % n2) for k in ks} == {(r1, r2) for r1 in (0, (n1 - 1) // 2, n1 - 1) for r2 in (0, n2 - 1)}
    case = LF.cut_case(length)
    assert len(case.rows) == 6
    for m in LF.CUT_METHODS:
        for key, row in case.corr.items():
            assert PP.decided(row, length, LF.FS, m, 1.0, LF.CUT_MED, case.records[m][key]), (length, m, key)
