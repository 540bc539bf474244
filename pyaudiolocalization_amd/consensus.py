"""Loop-closure consensus over several candidate peaks per pair: the device rule (csrc/consensus.hip, pal_tdoa_consensus*) in NumPy.

The closure check (closure.py) says which pairs of a TDOA table are wrong; it cannot put them right.  The right lag is usually in the
pair's GCC-PHAT row already, as its second or third peak.  Given K candidate peaks per pair, this rule picks per pair the candidate the
other pairs' candidates agree with, in the integer arithmetic of the closure check.  Per frame of M microphones and length L:

- ``cand_k[P][K]``: array indices, row-major over pairs i<j, ordered as the selection orders them (highest peak first); ``-1`` = absent;
  1 <= K <= 8; the present candidates of a pair form a prefix and candidate 0 is present;
- ``lag(p, c) = cand_k[p][c] - (L - 1)``; ``s(x, y, a)`` is ``lag({x, y}, a)`` for x < y and its negative for x > y (``cube``);
- **stage 0**: ``support[p][c]`` of pair p = (i, j) and a present candidate c: the number of third microphones k not in {i, j} for which a
  present candidate a of pair {i, k} and a present candidate b of pair {j, k} exist with ``|s(i,k,a) - s(j,k,b) - lag(p,c)| <= tol``;
  ``sel_0[p]``: the smallest c with the largest support;
- **rounds r = 1 .. rounds** (Jacobi: every pair of round r reads ``sel_{r-1}``): ``A`` the antisymmetric matrix of the lags chosen by
  ``sel_{r-1}`` (closure.lag_matrix), ``v[p][c]`` the number of k not in {i, j} with ``|A[i][k] - A[j][k] - lag(p,c)| <= tol`` (for the chosen
  candidate exactly its closure vote); ``sel_r[p] = sel_{r-1}[p]`` if its v is maximal, otherwise the smallest c with maximal v.  Exactly
  ``rounds`` rounds run: no early exit; at a fixed point they change nothing;
- ``summary``: ``moved`` pairs with sel != 0, closed triangles of candidate 0 and of the result (closure.summary at ``tol``), and the pairs
  that changed in the last round (in stage 0 against candidate 0 when ``rounds`` = 0).

Everything is integer arithmetic (int64 here, int32 on the device), so the two are compared byte for byte.  What the rule cannot see: among
two consistent sources (the source and an image source) the rounds converge on the one the majority of first picks lies on, whichever it
is; and a constant clock offset of one microphone closes every triangle, as in closure.py.
"""
from __future__ import annotations

import numpy as np

from . import closure
from ._ffi import BR_CONSENSUS, MAX_CANDIDATES, RECORD                  # PAL_BR_CONSENSUS, PAL_MAX_CANDIDATES

MAX_ROUNDS = 8                                                          # PAL_MAX_CONSENSUS_ROUNDS
ABSENT = -1
_FAR = 1 << 40                                                          # in place of a difference that has no present candidates: never within tol

# one row of the summary (pal_consensus_frame, 16 bytes)
SUMMARY = np.dtype([("moved", "<i4"), ("closed_before", "<i4"), ("closed_after", "<i4"), ("changed_last", "<i4")])
assert SUMMARY.itemsize == 16
OUTPUTS = ("sel", "table_out", "summary")                               # the order of the C ABI's three output pointers


def check_args(nframes, m, k, lengths, tol, rounds):
    """The argument checks of pal_tdoa_consensus* that need no data -> lengths[B] as int32; ValueError otherwise."""
    nframes, m, k, tol, rounds = int(nframes), int(m), int(k), int(tol), int(rounds)
    if nframes < 1:
        raise ValueError("need at least one frame")
    if not closure.MIN_MICS <= m <= closure.MAX_MICS:
        raise ValueError(f"the consensus takes {closure.MIN_MICS}..{closure.MAX_MICS} microphones (got {m})")
    if not 1 <= k <= MAX_CANDIDATES:
        raise ValueError(f"candidates per pair {k} outside 1..{MAX_CANDIDATES}")
    if not 0 <= tol <= closure.MAX_TOL:
        raise ValueError(f"tol {tol} outside 0..2^20")
    if not 0 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"rounds {rounds} outside 0..{MAX_ROUNDS}")
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (nframes,))
    if np.any(ln < 1) or np.any(ln > closure.MAX_LENGTH):
        raise ValueError("a frame length outside 1..2^24")
    return np.ascontiguousarray(ln, dtype=np.int32)


def check_candidates(cand_k, length: int) -> np.ndarray:
    """cand_k[P][K] of one frame -> the same as int64; ValueError for a present candidate outside 0..2 length - 2, an absent
    candidate 0 or a gap in the prefix of present candidates."""
    ck = np.asarray(cand_k, dtype=np.int64)
    present = ck != ABSENT
    if np.any(present & ((ck < 0) | (ck > 2 * int(length) - 2))):
        raise ValueError(f"a candidate outside 0..{2 * int(length) - 2}")
    if not np.all(present[:, 0]):
        raise ValueError("candidate 0 of a pair is absent")
    if np.any(present[:, 1:] & ~present[:, :-1]):
        raise ValueError("the present candidates of a pair must form a prefix")
    return ck


def centred(cand_k, length: int) -> np.ndarray:
    """Array indices as the pair pipeline reports them -> indices whose lag ``k - (L - 1)`` is the true delay d_j - d_i in samples.
    The pipeline keeps the reference's mapping: its rows are circular correlations of n = 2L - 1 samples with zero lag at
    index 0, so index k holds the circular lag t = k (k < L) or k - n, while the reported lag is k - (L - 1) - and three reported lags
    around a triangle sum to about +-L, never to 0.  The closure check and the consensus need the centred form: (L - 1) - t (the sign
    turns because the correlation of rows (i, j) peaks at d_i - d_j).  Absent entries (-1) stay."""
    ck = np.asarray(cand_k, dtype=np.int64)
    length = int(length)
    t = np.where(ck < length, ck, ck - (2 * length - 1))
    return np.where(ck == ABSENT, ABSENT, (length - 1) - t)


def cube(cand_k, length: int, m: int):
    """cand_k[P][K] -> (s[m][m][K] int64 with s[x][y][a] = lag({x,y}, a) for x < y and its negative for x > y, present[m][m][K])."""
    m = int(m)
    ck = np.asarray(cand_k, dtype=np.int64)
    k = ck.shape[1]
    s = np.zeros((m, m, k), dtype=np.int64)
    present = np.zeros((m, m, k), dtype=bool)
    p = 0
    for i in range(m):
        for j in range(i + 1, m):
            for a in range(k):
                if ck[p][a] != ABSENT:
                    lag = int(ck[p][a]) - (int(length) - 1)
                    s[i, j, a], s[j, i, a] = lag, -lag
                    present[i, j, a] = present[j, i, a] = True
            p += 1
    return s, present


def _first_max(counts, present) -> int:
    """The smallest present c with the largest count."""
    best = -1
    for c in range(len(counts)):
        if present[c] and (best < 0 or counts[c] > counts[best]):
            best = c
    return best


def support(cand_k, length: int, m: int, tol: int = 1, first=None) -> np.ndarray:
    """Stage 0: support[P][K] (int32; -1 for an absent candidate) of one frame.  ``first``: only the pairs (i, j > i) of these
    microphones i are computed (the other rows stay -1)."""
    m, tol = int(m), int(tol)
    ck = np.asarray(cand_k, dtype=np.int64)
    s, present = cube(ck, length, m)
    out = np.full(ck.shape, -1, dtype=np.int32)
    kk = ck.shape[1]
    step = max(1, (1 << 17) // (m * kk * kk))                                           # pairs per block: the block's [j][k][a b] stays in cache
    p = 0
    for i in range(m - 1):                                                              # microphone i by microphone i, as closure.votes
        if first is not None and i not in first:
            p += m - 1 - i
            continue
        for j0 in range(i + 1, m, step):
            j = np.arange(j0, min(j0 + step, m))
            diff = (s[i][None, :, :, None] - s[j][:, :, None, :]).reshape(j.shape[0], m, kk * kk)      # [j][k][a b]
            valid = (present[i][None, :, :, None] & present[j][:, :, None, :]).reshape(diff.shape)     # k = i and k = j: nothing present
            diff[~valid] = _FAR
            rows = ck[p:p + j.shape[0]]
            for c in range(kk):
                lag = rows[:, c] - (int(length) - 1)
                hit = np.abs(diff - lag[:, None, None]) <= tol
                count = np.count_nonzero(hit.any(axis=2), axis=1)
                out[p:p + j.shape[0], c] = np.where(rows[:, c] != ABSENT, count, -1)
            p += j.shape[0]
    return out


def stage0(cand_k, length: int, m: int, tol: int = 1) -> np.ndarray:
    """sel_0[P] (int32): per pair the smallest candidate with the largest support."""
    ck = np.asarray(cand_k, dtype=np.int64)
    sup = support(ck, length, m, tol)
    return np.array([_first_max(sup[p], ck[p] != ABSENT) for p in range(ck.shape[0])], dtype=np.int32)


def chosen_k(cand_k, sel) -> np.ndarray:
    """k_sel[P] of the table that ``sel`` chooses."""
    ck = np.asarray(cand_k, dtype=np.int64)
    return ck[np.arange(ck.shape[0]), np.asarray(sel, dtype=np.int64)]


def round_votes(cand_k, sel, length: int, m: int, tol: int = 1) -> np.ndarray:
    """v[P][K] (int32; -1 for an absent candidate) of one round that reads ``sel``."""
    m, tol = int(m), int(tol)
    ck = np.asarray(cand_k, dtype=np.int64)
    a = closure.lag_matrix(chosen_k(ck, sel) - (int(length) - 1), m)
    third = np.arange(m)
    out = np.full(ck.shape, -1, dtype=np.int32)
    p = 0
    for i in range(m - 1):
        j = np.arange(i + 1, m)
        d = a[i][None, :] - a[j]                                                        # [j][k]
        others = (third[None, :] != i) & (third[None, :] != j[:, None])                 # k not in {i, j}
        rows = ck[p:p + j.shape[0]]
        for c in range(ck.shape[1]):
            lag = rows[:, c] - (int(length) - 1)
            count = np.count_nonzero((np.abs(d - lag[:, None]) <= tol) & others, axis=1)
            out[p:p + j.shape[0], c] = np.where(rows[:, c] != ABSENT, count, -1)
        p += j.shape[0]
    return out


def one_round(cand_k, sel, length: int, m: int, tol: int = 1) -> np.ndarray:
    """sel_r[P] from sel_{r-1}[P]: a pair keeps its candidate if its v is maximal, otherwise takes the smallest c with maximal v."""
    ck = np.asarray(cand_k, dtype=np.int64)
    v = round_votes(ck, sel, length, m, tol)
    out = np.array(sel, dtype=np.int32)
    for p in range(ck.shape[0]):
        best = _first_max(v[p], ck[p] != ABSENT)
        if v[p][out[p]] < v[p][best]:
            out[p] = best
    return out


def consensus_frame(cand_k, length: int, m: int, tol: int = 1, rounds: int = 2, sel0=None):
    """One frame -> (sel[P] int32, summary of SUMMARY).  ``sel0``: stage 0's result, where the caller has it already."""
    ck = check_candidates(cand_k, length)
    if ck.ndim != 2 or ck.shape[0] != int(m) * (int(m) - 1) // 2:
        raise ValueError("cand_k must have M (M - 1) / 2 rows of K candidates")
    sel = stage0(ck, length, m, tol) if sel0 is None else np.array(sel0, dtype=np.int32)
    prev = np.zeros_like(sel)
    for _ in range(int(rounds)):
        prev, sel = sel, one_round(ck, sel, length, m, tol)
    rec = np.zeros((), dtype=SUMMARY)
    rec["moved"] = int(np.count_nonzero(sel))
    for name, chosen in (("closed_before", ck[:, 0]), ("closed_after", chosen_k(ck, sel))):
        rec[name] = closure.summary(closure.votes(closure.lags(chosen, length), m, tol), m)["closed"]
    rec["changed_last"] = int(np.count_nonzero(sel != prev))
    return sel, rec


def apply(tables, cand_k, cand_h, sel) -> np.ndarray:
    """table_out: the records with k_sel the chosen candidate, sel_height its height (when ``cand_h`` is given) and PAL_BR_CONSENSUS set
    where sel != 0; everything else copied."""
    out = np.array(tables, dtype=RECORD, copy=True)
    ck = np.asarray(cand_k, dtype=np.int64).reshape(-1, np.shape(cand_k)[-1])
    flat, pick = out.reshape(-1), np.asarray(sel, dtype=np.int64).reshape(-1)
    rows = np.arange(flat.shape[0])
    flat["k_sel"] = ck[rows, pick]
    if cand_h is not None:
        flat["sel_height"] = np.asarray(cand_h, dtype=np.float64).reshape(ck.shape)[rows, pick]
    flat["branch"] |= np.where(pick != 0, BR_CONSENSUS, 0).astype(np.int32)
    return out


def tdoa_consensus(cand_k, lengths, m: int, tol: int = 1, rounds: int = 2):
    """cand_k[B][P][K] (or [P][K]), lengths[B] (or one length) -> (sel[B][P] int32, summary[B] of SUMMARY): what Engine.tdoa_consensus
    computes, frame by frame."""
    ck = np.asarray(cand_k, dtype=np.int64)
    if ck.ndim == 2:
        ck = ck[None]
    if ck.ndim != 3:
        raise ValueError("cand_k must be [P][K] or [B][P][K]")
    m = int(m)
    ln = check_args(ck.shape[0], m, ck.shape[2], lengths, tol, rounds)
    if ck.shape[1] != m * (m - 1) // 2:
        raise ValueError("cand_k must have M (M - 1) / 2 rows per frame")
    sel = np.zeros(ck.shape[:2], dtype=np.int32)
    summ = np.zeros(ck.shape[0], dtype=SUMMARY)
    for b in range(ck.shape[0]):
        sel[b], summ[b] = consensus_frame(ck[b], int(ln[b]), m, tol, rounds)
    return sel, summ
