"""The designed rows of tests/peak_positions.py and the oracle they are judged by, without a GPU: every designed pair has its
maximum at its designed index, the rows are decided (no integer field of the oracle's record changes under a perturbation of
1e-11 max|corr|), they keep their distance from the finishing pass's energy rule, the windowed calls reach both the plain
branch and the window retry, and the two-arrival rows do what their names say.  Frame lengths: those of
test_gpu_peak_positions.py up to 12 000, with the plan factors that test confirms on the device written out here."""
import numpy as np
import pytest

from oracle import pal_oracle as O

import peak_positions as P

# (L, n1, n2, borders of the stored-row passes as well)
SHAPES = [(11437, 89, 257, False), (8193, 5, 3277, False), (8538, 25, 683, False), (1008, 5, 403, False), (11962, 47, 509, False),
          (12000, 103, 233, True), (6007, 0, 0, True), (2500, 0, 0, True), (1000, 0, 0, True)]


def test_designed_indices_by_hand():
    """L = 8538 = (25 x 683 + 1) / 2 at 16 kHz, 20 ms: w = 320, distance 16."""
    L, n1, n2 = 8538, 25, 683
    n, c = 2 * L - 1, L - 1
    assert P.window_half_width(16000.0, 0.02) == 320 and P.window_half_width(8000.0, 0.01) == 80
    got = set(P.designed_indices(L, n1, n2, 16000.0, 0.02))
    assert {0, 1, 2, n - 3, n - 2, n - 1, c - 1, c, c + 1} <= got
    assert {c - 320, c + 320, c - 321, c + 321, c - 306, c + 306, c - 304, c + 304, c - 335, c + 335} <= got
    for r1 in (0, 1, 12, 13, 24):
        for r2 in (0, 1, 681, 682, 61, 62, 63, 124, 247, 248, 249):
            hits = [m for m in got if m % n1 == r1 and m % n2 == r2]
            assert len(hits) >= 1, (r1, r2)
    assert len(got) <= 9 + 10 + 55
    stored = set(P.designed_indices(6007, 0, 0, 16000.0, 0.02, stored=True))
    assert {63, 64, 65, 255, 256, 257, 1363, 1364, 1365, 5455, 5456, 5457, 11967, 11968, 11969, 10911, 10912, 10913} <= stored
    assert max(stored) == 2 * 6007 - 2
    assert set(P.designed_indices(500, 1, 999, 8000.0, 0.01)) >= {61, 62, 63, 997, 998}    # one row: the column residues alone


def test_star_frames_reach_every_index():
    L = 700
    idx = sorted(set(range(0, 2 * L - 1, 13)) | {L - 2, L - 1, L, 2 * L - 2})               # 109 indices: three frames and more
    star = P.star_frames(L, idx, 3)
    assert star.frames.shape[1] <= P.MAX_MICS and len({f.shape for f in star.frames}) == 1
    assert sorted(k for d in star.designed for k in d.values()) == idx
    again = P.star_frames(L, idx, 3)
    assert np.array_equal(star.frames, again.frames)
    for f, frame in enumerate(star.frames):
        for j, k in list(star.designed[f].items())[:4]:
            assert int(np.argmax(O.phat_correlation(frame[0], frame[j]))) == k
        (i, j), k = sorted(star.implied[f].items())[-1]
        assert int(np.argmax(O.phat_correlation(frame[i], frame[j]))) == k


@pytest.mark.parametrize("L,n1,n2,stored", SHAPES, ids=[f"L{s[0]}" for s in SHAPES])
def test_designed_rows_in_the_oracle(L, n1, n2, stored):
    fs, med = P.rates(L)
    c = P.case(L, n1, n2, fs, med, stored)
    f, i, j, _ = c.designed_rows[0]
    assert np.array_equal(c.corr(f, i, j), O.phat_correlation(c.star.frames[f, i], c.star.frames[f, j]))   # the shared spectra change nothing
    undecided = 0
    branches = set()
    for f, i, j, k in c.designed_rows:
        share = P.outside_energy_share(c.corr(f, i, j))
        # the pass hands a row on below 0.25: a factor of two
        assert share >= 0.5, (L, k, share)
        for method, mult, m in P.param_sets(med):
            want = c.want(f, i, j, method, mult, m)
            assert want["k_argmax"] == k, (L, k, method, mult, m, want)
            undecided += not want["decided"]
            if m is not None:
                branches.add(want["branch"])
    assert undecided <= P.UNDECIDED_SHARE * 6 * len(c.designed_rows), (L, undecided)
    assert {0, O.BR_WINDOW_RETRY} <= branches, (L, sorted(branches))
    c.release()


@pytest.mark.parametrize("L", [11962, 2500])
def test_two_arrival_rows_in_the_oracle(L):
    fs, med = P.rates(L)
    w, d, c = P.window_half_width(fs, med), int(fs * 0.001), L - 1
    ta = P.two_arrival_frames(L, fs, med, L)
    assert ta.frames.shape == (2 * P.TWO_ARRIVAL_COPIES, 4, L)
    assert [r[2] for r in ta.rows] == ["outside", "inside", "apart"] * 2 * P.TWO_ARRIVAL_COPIES
    for f, j, name, strong, weak in ta.rows:
        corr = O.phat_correlation(ta.frames[f, 0], ta.frames[f, j])
        inside = lambda k: abs(k - c) <= w
        assert abs(strong - weak) == (d if name == "apart" else d - 1)
        assert inside(strong) == (name == "inside") and inside(weak) != (name == "inside")
        for method, mult in P.MODES:
            want = P.record(corr, L, fs, method, mult, med)
            tag = (L, f, name, method, mult, want)
            assert P.decided(corr, L, fs, method, mult, med, want), tag
            assert want["k_argmax"] == strong, tag
            if name == "outside":                                   # the weak peak is suppressed: a noise peak elsewhere in the window
                assert inside(want["k_sel"]) and want["k_sel"] not in (strong, weak), tag
            else:
                assert want["k_sel"] == (strong if name == "inside" else weak), tag
