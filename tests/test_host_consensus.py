"""The consensus specification (pyaudiolocalization_amd/consensus.py) on the CPU: against a plain loop over (p, c, k, a, b), on random
candidate tables whose true lag sits in a random slot, on two consistent sources (the source and an image source), the identities that
tie it to the closure check, the recorded stage 0 of the 256-microphone frame, and the argument checks."""
import numpy as np
import pytest

import consensus_tables as CS
import robust_tables as T
from pyaudiolocalization_amd import closure as CL
from pyaudiolocalization_amd import consensus as CN


def _pairs(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


def _signed(cand, index, x, y, a, length):
    """s(x, y, a), or None where the candidate is absent."""
    k = cand[index[min(x, y), max(x, y)]][a]
    if k == CN.ABSENT:
        return None
    lag = int(k) - (length - 1)
    return lag if x < y else -lag


def _brute_stage0(cand, m, length, tol):
    pairs = _pairs(m)
    index = {pair: p for p, pair in enumerate(pairs)}
    kk = cand.shape[1]
    sel = []
    for p, (i, j) in enumerate(pairs):
        best, best_support = -1, -1
        for c in range(kk):
            if cand[p][c] == CN.ABSENT:
                continue
            lag = int(cand[p][c]) - (length - 1)
            support = 0
            for k in range(m):
                if k in (i, j):
                    continue
                hit = False
                for a in range(kk):
                    for b in range(kk):
                        sa, sb = _signed(cand, index, i, k, a, length), _signed(cand, index, j, k, b, length)
                        if sa is not None and sb is not None and abs(sa - sb - lag) <= tol:
                            hit = True
                support += hit
            if support > best_support:
                best, best_support = c, support
        sel.append(best)
    return np.array(sel, dtype=np.int32)


def _brute_round(cand, sel, m, length, tol):
    pairs = _pairs(m)
    index = {pair: p for p, pair in enumerate(pairs)}
    out = []
    for p, (i, j) in enumerate(pairs):
        votes = {}
        for c in range(cand.shape[1]):
            if cand[p][c] == CN.ABSENT:
                continue
            lag = int(cand[p][c]) - (length - 1)
            votes[c] = sum(1 for k in range(m) if k not in (i, j) and
                           abs(_signed(cand, index, i, k, sel[index[min(i, k), max(i, k)]], length)
                               - _signed(cand, index, j, k, sel[index[min(j, k), max(j, k)]], length) - lag) <= tol)
        top = max(votes.values())
        out.append(sel[p] if votes[sel[p]] == top else min(c for c in votes if votes[c] == top))
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("m", [4, 5, 8])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_specification_equals_the_plain_loop(m, k):
    length = 50
    rng = np.random.default_rng([m, k])
    for tol in (0, 1, 3):
        cand = CS.ragged(rng.integers(-6, 7, (m * (m - 1) // 2, k)) + length - 1, tol)       # small lags: many chance agreements and ties
        sel = _brute_stage0(cand, m, length, tol)
        assert np.array_equal(CN.stage0(cand, length, m, tol), sel), (m, k, tol)
        assert np.array_equal(CN.tdoa_consensus(cand, length, m, tol, 0)[0][0], sel)
        for rounds in (1, 2, 3):
            before, sel = sel, _brute_round(cand, sel, m, length, tol)
            got, summary = CN.tdoa_consensus(cand, length, m, tol, rounds)
            assert np.array_equal(got[0], sel), (m, k, tol, rounds)
            assert summary[0]["changed_last"] == np.count_nonzero(sel != before)
            assert summary[0]["moved"] == np.count_nonzero(sel)


@pytest.mark.parametrize("case", CS.CASES)
def test_stage0_finds_the_true_slot(case):
    m = case[0]
    t = CS.random_candidates(*case)
    sel, summary = CS.spec(t["cand_k"], T.LENGTH, m, 1, 0)
    has = t["slot"] >= 0
    print(f"[consensus] {case}: {np.count_nonzero(t['slot'] == 0)} of {has.size} first picks right, closed triangles "
          f"{summary[0]['closed_before']} -> {summary[0]['closed_after']}")
    assert np.array_equal(sel[0][has], t["slot"][has])
    assert summary[0]["closed_after"] > summary[0]["closed_before"]
    assert summary[0]["changed_last"] == summary[0]["moved"] == np.count_nonzero(sel)


@pytest.mark.parametrize("case", CS.TWO_SOURCE_CASES)
def test_two_consistent_sources(case):
    m = case[0]
    t = CS.two_sources(*case)
    sel, _ = CS.spec(t["cand_k"], T.LENGTH, m, 1, 0)
    assert np.all(sel == 0)                                                              # stage 0 ties: both lags get M - 2 supports
    sel, summary = CS.spec(t["cand_k"], T.LENGTH, m, 1, 4)
    lag = CN.chosen_k(t["cand_k"], sel[0]) - (T.LENGTH - 1)
    differ = t["true_lag"] != t["image_lag"]
    print(f"[consensus] {case}: {np.count_nonzero(t['first'])} of {differ.size} first picks on the source, summary {summary[0]}")
    assert summary[0]["changed_last"] == 0
    assert np.array_equal(lag[differ], t["true_lag"][differ])
    for rounds in (5, 8):                                                                # a fixed point: further rounds change nothing
        assert np.array_equal(CS.spec(t["cand_k"], T.LENGTH, m, 1, rounds)[0], sel)


def test_one_candidate_is_the_identity():
    for m, seed in ((4, 5), (16, 3)):
        t = T.table(m, seed, m)
        for rounds in (0, 2):
            sel, summary = CN.tdoa_consensus(t["k_sel"][:, None], T.LENGTH, m, 1, rounds)
            assert np.all(sel == 0)
            closed = CL.tdoa_closure(t["k_sel"], T.LENGTH, m, 1)[3][0]["closed"]
            assert summary[0].tolist() == (0, closed, closed, 0)


@pytest.mark.parametrize("case", CS.CASES[2:])
def test_closed_after_is_the_closure_summary_of_the_result(case):
    m = case[0]
    t = CS.random_candidates(*case)
    cand = CS.ragged(t["cand_k"], 3)
    for tol, rounds in ((0, 1), (1, 2), (5, 0)):
        sel, summary = CS.spec(cand, T.LENGTH, m, tol, rounds)
        after = CL.tdoa_closure(CN.chosen_k(cand, sel[0]), T.LENGTH, m, tol)[3][0]["closed"]
        before = CL.tdoa_closure(cand[:, 0], T.LENGTH, m, tol)[3][0]["closed"]
        assert (summary[0]["closed_before"], summary[0]["closed_after"]) == (before, after)
        tab = CN.apply(np.zeros(cand.shape[0], dtype=CN.RECORD), cand, None, sel[0])
        assert np.array_equal(tab["k_sel"], CN.chosen_k(cand, sel[0]))
        assert np.array_equal(tab["branch"], np.where(sel[0] != 0, CN.BR_CONSENSUS, 0))


def test_recorded_stage0_of_the_256_microphone_frame():
    """tests/golden/consensus_m256.npz against the specification on the pairs of three microphones (first, middle, last but one)."""
    cand = CS.big_frame()
    m = CS.BIG["m"]
    with np.load(CS.BIG_GOLDEN) as z:
        sel0 = z["sel0"]
    assert sel0.shape == (m * (m - 1) // 2,) and cand.shape == (sel0.shape[0], 8)
    assert np.any(cand[:, 1:] == CN.ABSENT) and np.any(cand[:, 7] != CN.ABSENT)
    first = (0, 100, m - 2)
    sup = CN.support(cand, T.LENGTH, m, CS.BIG["tol"], first=first)
    checked = 0
    for i in first:
        p0 = i * m - i * (i + 1) // 2 - i - 1
        for p in range(p0 + i + 1, p0 + m):
            assert sel0[p] == CN._first_max(sup[p], cand[p] != CN.ABSENT), p
            checked += 1
    assert checked == 255 + 155 + 1
    sel, summary = CS.big_spec(2)
    assert summary[0]["closed_after"] > summary[0]["closed_before"] and summary[0]["moved"] == np.count_nonzero(sel)


def test_argument_errors():
    t = CS.random_candidates(4, 5, .3, 2, 0)
    good = dict(cand_k=t["cand_k"], lengths=T.LENGTH, m=4, tol=1, rounds=2)
    CN.tdoa_consensus(**good)

    def changed(p, c, value):
        ck = t["cand_k"].copy()
        ck[p, c] = value
        return ck
    for change in (dict(m=2), dict(m=257), dict(m=5), dict(tol=-1), dict(tol=(1 << 20) + 1), dict(rounds=-1), dict(rounds=9),
                   dict(lengths=0), dict(lengths=(1 << 24) + 1), dict(cand_k=np.zeros((6, 0), dtype=np.int64)),
                   dict(cand_k=np.zeros((6, 9), dtype=np.int64)), dict(cand_k=np.zeros((1, 1, 6, 2), dtype=np.int64)),
                   dict(cand_k=np.zeros((0, 6, 2), dtype=np.int64)),
                   dict(cand_k=changed(2, 1, 2 * T.LENGTH - 1)), dict(cand_k=changed(5, 0, -2)), dict(cand_k=changed(3, 0, -1)),
                   dict(cand_k=np.concatenate([changed(1, 1, -1), t["cand_k"][:, :1]], axis=1))):
        with pytest.raises(ValueError):
            CN.tdoa_consensus(**{**good, **change})
    CN.tdoa_consensus(**{**good, "cand_k": changed(1, 1, -1)})                               # an absent last candidate is valid
    CN.tdoa_consensus(**{**good, "cand_k": changed(0, 0, 2 * T.LENGTH - 2)})                 # the last valid index
