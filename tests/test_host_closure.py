"""The loop-closure specification (pyaudiolocalization_amd/closure.py) on the CPU: against a plain triple loop over the triangles, on the
clean and outlier tables of tests/robust_tables.py, its counting identities on random tables, the linear solve under its soft weights,
the dead-microphone tables and the argument checks."""
import numpy as np
import pytest

import closure_tables as CT
import robust_tables as T
from pyaudiolocalization_amd import closure as CL
from pyaudiolocalization_amd import solve as S


def _triple_loop(lag, m, tol):
    """votes, mic_closed, closed straight from the definition: every triangle x < y < z once."""
    index = {}
    for i in range(m):
        for j in range(i + 1, m):
            index[i, j] = len(index)
    votes = np.zeros(len(index), dtype=np.int64)
    per_mic = np.zeros(m, dtype=np.int64)
    closed = 0
    for x in range(m):
        for y in range(x + 1, m):
            for z in range(y + 1, m):
                if abs(int(lag[index[x, y]]) + int(lag[index[y, z]]) - int(lag[index[x, z]])) <= tol:
                    closed += 1
                    for pair in ((x, y), (y, z), (x, z)):
                        votes[index[pair]] += 1
                    per_mic[[x, y, z]] += 1
    return votes, per_mic, closed


@pytest.mark.parametrize("m", [3, 4, 5, 8])
def test_specification_equals_the_triple_loop(m):
    for tol, span in ((0, 3), (1, 6), (5, 20)):
        k_sel = CT.random_tables(6, m, 100 + tol, span)
        votes, per_mic, _, summary = CL.tdoa_closure(k_sel, T.LENGTH, m, tol)
        for b in range(k_sel.shape[0]):
            want_v, want_m, want_c = _triple_loop(k_sel[b] - (T.LENGTH - 1), m, tol)
            assert np.array_equal(votes[b], want_v) and np.array_equal(per_mic[b], want_m), (m, tol, b)
            assert summary[b]["closed"] == want_c and summary[b]["triangles"] == m * (m - 1) * (m - 2) // 6
            assert summary[b]["worst_mic"] == int(np.argmin(want_m))
        assert 0 < summary["closed"].sum() < summary["triangles"].sum(), (m, tol)      # the tables close some triangles and break some


def test_clean_table_gets_every_vote():
    t = T.table(8, 2, 0)
    votes, per_mic, weights, summary = CT.spec(t["k_sel"], T.LENGTH, 8)
    assert np.all(votes == 6) and np.all(per_mic == 21) and np.all(weights == 1.0)
    assert summary[0].tolist() == (56, 56, 28, 0)


@pytest.mark.parametrize("case", T.OUTLIER_CASES)
def test_zero_vote_pairs_are_the_replaced_pairs(case):
    t = T.table(*case)
    votes, _, weights, summary = CT.spec(t["k_sel"], T.LENGTH, case[0])
    wrong = t["bad"][np.abs(t["lag"] - t["true_lag"])[t["bad"]] > 1]
    assert wrong.size > 0
    assert set(np.flatnonzero(votes[0] == 0)) == set(wrong)
    assert np.all(np.delete(votes[0], wrong) >= 1)
    assert summary[0]["kept_pairs"] == votes.shape[1] - wrong.size == np.count_nonzero(weights[0])


def test_counting_identities_on_random_tables():
    for m, b, span, tol in ((3, 40, 2, 1), (7, 20, 5, 1), (16, 8, 10, 2), (33, 3, 40, 5)):
        k_sel = CT.random_tables(b, m, 7, span)
        votes, per_mic, _, summary = CL.tdoa_closure(k_sel, T.LENGTH, m, tol)
        pi, pj = S.pair_indices(m)
        for f in range(b):
            assert votes[f].sum() == 3 * summary[f]["closed"]
            for mic in range(m):
                assert 2 * per_mic[f][mic] == votes[f][(pi == mic) | (pj == mic)].sum()


@pytest.mark.parametrize("case", T.OUTLIER_CASES)
def test_linear_solve_with_soft_weights_finds_the_source(case):
    """The unweighted linear solve is more than a metre off on these tables (tests/test_host_solve_loss.py pins that)."""
    t = T.table(*case)
    weights = CT.spec(t["k_sel"], T.LENGTH, case[0])[2][0]
    rec = S.solve_frame(t["k_sel"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights=weights, buffer=T.BUFFER, grid=T.GRID)
    dist = float(np.linalg.norm(rec["position"] - T.SRC))
    print(f"[closure] {case}: linear solve under the soft closure weights {dist:.4f} m from the source")
    assert rec["status"] & S.ST_CONVERGED
    assert dist < 0.15, case


@pytest.mark.parametrize("case", CT.DEAD_CASES)
def test_dead_microphone_is_the_worst(case):
    m, _, mic = case
    t = CT.dead_table(*case)
    _, per_mic, _, summary = CT.spec(t["k_sel"], T.LENGTH, m)
    print(f"[closure] {case}: the dead microphone closes {per_mic[0][mic]} of {(m - 1) * (m - 2) // 2} triangles, the others {sorted(set(np.delete(per_mic[0], mic)))}")
    assert summary[0]["worst_mic"] == mic
    assert per_mic[0][mic] <= 1
    assert np.all(np.delete(per_mic[0], mic) >= (m - 2) * (m - 3) // 2)              # every triangle without the dead microphone closes


def test_weight_modes_and_min_votes():
    votes = np.array([0, 1, 2, 6, 5, 0], dtype=np.int32)                             # any six vote counts of a four-microphone table's shape
    assert CL.weights(votes, 8, 0, "mask").tolist() == [1, 1, 1, 1, 1, 1]
    assert CL.weights(votes, 8, 2, "mask").tolist() == [0, 0, 1, 1, 1, 0]
    assert CL.weights(votes, 8, 2, "soft").tolist() == [0, 0, 2 / 6, 6 / 6, 5 / 6, 0]
    assert CL.weights(votes, 8, 7, "soft").tolist() == [0] * 6                        # above M - 2: valid, nothing kept
    t = T.table(8, 2, 4)
    for min_votes, mode in ((0, "mask"), (0, "soft"), (6, "soft"), (7, "mask")):
        v, _, w, s = CL.tdoa_closure(t["k_sel"], T.LENGTH, 8, 1, min_votes, mode)
        assert s[0]["kept_pairs"] == np.count_nonzero(w[0] > 0)
    assert CL.tdoa_closure(t["k_sel"], T.LENGTH, 8, 1, 0, "mask")[3][0]["kept_pairs"] == 28
    assert CL.tdoa_closure(t["k_sel"], T.LENGTH, 8, 1, 0, "soft")[3][0]["kept_pairs"] == 24      # a zero vote is a zero weight
    assert CL.tdoa_closure(t["k_sel"], T.LENGTH, 8, 1, 7, "mask")[3][0]["kept_pairs"] == 0


def test_argument_errors():
    t = T.table(4, 5, 1)
    k = t["k_sel"]
    good = dict(k_sel=k, lengths=T.LENGTH, m=4, tol=1, min_votes=1, mode="soft")
    CL.tdoa_closure(**good)
    for change in (dict(m=2, k_sel=k[:1]), dict(m=257, k_sel=np.zeros(257 * 128, dtype=np.int64)), dict(m=5), dict(tol=-1), dict(tol=(1 << 20) + 1),
                   dict(min_votes=-1), dict(mode="hard"), dict(mode=None), dict(lengths=0), dict(lengths=(1 << 24) + 1),
                   dict(k_sel=np.where(np.arange(6) == 2, 2 * T.LENGTH - 1, k)), dict(k_sel=np.where(np.arange(6) == 5, -1, k)),
                   dict(k_sel=np.zeros((1, 1, 6), dtype=np.int64))):
        with pytest.raises(ValueError):
            CL.tdoa_closure(**{**good, **change})
    with pytest.raises(ValueError):
        CL.empty_outputs(1, 4, ())
    with pytest.raises(ValueError):
        CL.empty_outputs(1, 4, ("votes", "lags"))
    from pyaudiolocalization_amd import stream
    mics = t["mics"]
    for kw in (dict(weights="closure", closure_tol=-1), dict(weights="closure", closure_mode="hard"), dict(weights="closure", closure_min_votes=-1),
               dict(weights="votes"), dict(weights=None)):
        with pytest.raises(ValueError):
            stream._solve_keywords(mics, T.FS, T.C_SOUND, None, **{**dict(weights="ones", buffer=5.0, grid=4, max_iter=200, loss="linear", f_scale=1.0), **kw})
    args = stream._solve_keywords(mics, T.FS, T.C_SOUND, None, "closure", 5.0, 4, 200, "linear", 1.0, 2, 3, "mask")
    assert (args["weights"], args["closure_tol"], args["closure_min_votes"], args["closure_mode"]) == ("closure", 2, 3, "mask")
    assert "closure_tol" not in stream._solve_keywords(mics, T.FS, T.C_SOUND, None, "snr", 5.0, 4, 200, "linear", 1.0)
