"""Preconditions of tests/test_gpu_rader_family.py, checked without a GPU, so that a failure there can only be the engine's.

* The cases are what tests/rader_family.py says they are: L = (991 N1 + 1) / 2, the chunk counts of the column passes, the
  exponents of the amplitude-sensitive variant, and unequal lengths that add up to n + 1 on the right side of the rule.
* Peak margins: for every case, window and method the oracle's selected peak and its argmax lead their runner-ups by
  ``row_scale.MARGIN`` (absolute: the rows are of unit scale).  A condition on the seeded inputs, not a tolerance: a seed that
  fails is replaced in ``rader_family.SEEDS``.  The pairs of the silent microphone are exact zero rows in the reference (pinned
  here) and have no peak to lead; the device test compares them with exact zeros.
* The amplitude-sensitive variant: with every microphone at 2^e, e = round(log2(1e-10 / L) / 2), the cross spectrum is of the
  size of the whitening's 1e-10, so the oracle's row moves by at least a tenth of the unscaled row's maximum (measured 0.43 ...
  0.66) and keeps its argmax.  An amplitude error in a forward spectrum therefore shows in the row: the whitening cannot hide it.
"""
import numpy as np
import pytest

import rader_family as RF
import row_scale as RS

NCH = {3: 1, 9: 1, 11: 1, 23: 1, 25: 2, 45: 2, 47: 3, 67: 3, 69: 4, 87: 4, 91: 5, 97: 5, 113: 6, 127: 6}
LENGTHS = {3: 1487, 9: 4460, 11: 5451, 23: 11397, 25: 12388, 45: 22298, 47: 23289, 67: 33199, 69: 34190, 87: 43109, 91: 45091,
           97: 48064, 113: 55992, 127: 62929}


def test_cases_are_the_issue_s_table():
    assert sorted(RF.N1S) == sorted(NCH) == sorted(LENGTHS)
    for n1 in RF.N1S:
        assert RF.length_of(n1) == LENGTHS[n1] and 2 * RF.length_of(n1) - 1 == n1 * RF.N2
        assert RF.chunks(n1) == NCH[n1]
        assert RF.column_kernel(n1) == ("k_pfa_cols_stats" if n1 <= 23 else "k_pfa_cols_fin" if n1 <= 87 else "k_pfa_cols")
    assert [RF.amplitude_exponent(n1) for n1 in RF.AMPLITUDE] == [-22, -23, -24, -25]
    assert min(RF.amplitude_exponent(n1) for n1 in RF.N1S) == -25 and max(RF.amplitude_exponent(n1) for n1 in RF.N1S) == -22
    for n1 in RF.UNEQUAL:
        n, h = RF.N2 * n1, RF.half(n1)
        for tag, len1, len2, launches in RF.unequal_cases(n1):
            assert len1 >= 1 and len2 >= 1 and len1 + len2 - 1 == n, (n1, tag)
            cut = [(ln - 1) // RF.N2 <= h for ln in (len1, len2)]
            if launches is not None:
                assert sum(cut) == launches, (n1, tag, cut)
        assert RF.unequal_cases(n1)[0][1] == RF.N2 * (h + 1) and (RF.unequal_cases(n1)[0][1] - 1) // RF.N2 == h
        assert (RF.unequal_cases(n1)[1][1] - 1) // RF.N2 == h + 1


@pytest.mark.parametrize("n1,shape", RF.SHAPE_CASES, ids=["N1=%d-%s" % c for c in RF.SHAPE_CASES])
def test_peak_margins(n1, shape):
    b, m = RF.SHAPES[shape]
    fr = RF.frames(n1, shape)
    assert fr.shape == (b, m, RF.length_of(n1))
    worst = np.inf
    for f in range(b):
        for i, j in RS.pairs_of(m):
            if RF.silent_pair(shape, f, i, j):
                assert not RF.oracle_corr(n1, shape, f, i, j).any()
                continue
            for med in RF.MEDS:
                for method in RF.METHODS:
                    mg = RF.peak_margin(n1, shape, f, i, j, med, method)
                    assert mg > RS.MARGIN, (n1, shape, f, i, j, med, method, mg)
                    worst = min(worst, mg)
    print("N1 = %d %s: smallest peak margin %.3g" % (n1, shape, worst))


@pytest.mark.parametrize("n1", RF.AMPLITUDE)
def test_amplitude_sensitive_variant_moves_the_oracle_row(n1):
    e = RF.amplitude_exponent(n1)
    for k, (i, j) in enumerate(RS.pairs_of(3)):
        plain, scaled = RF.oracle_corr(n1, "narrow", 0, i, j), RF.oracle_corr(n1, "narrow", 0, i, j, e)
        moved = float(np.max(np.abs(scaled - plain)) / np.max(np.abs(plain)))
        print("N1 = %d pair (%d, %d) at 2^%d: the row moves by %.3g of its maximum" % (n1, i, j, e, moved))
        if k == 0:
            assert moved >= 0.1, (n1, e, moved)
        assert int(np.argmax(scaled)) == int(np.argmax(plain)), (n1, i, j)
        top = np.sort(scaled)[-2:]
        assert top[1] - top[0] > RS.MARGIN, (n1, i, j, float(top[1] - top[0]))   # (the device test compares the argmax as well)
