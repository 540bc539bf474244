"""The device bootstrap at its edge shapes (csrc/bootstrap.hip, csrc/bootstrap_map.h; shapes: tests/bootstrap_shapes.py).

k_bootstrap_shuffle against the specification (pyaudiolocalization_amd/bootstrap.py), bit for bit: lengths around its 256-lane
passes and 1024-sample workgroups, block sizes at which ShuffleMap's closed form degenerates, more rows than one launch holds,
counters beyond 32 bits, refusals.  bootstrap_peaks_dev against the oracle's PHAT of the specification's shuffles: tiny frames, the
transform routes, a round boundary at the default group size, the round that the 1 GiB cap cuts below one launch group, the forms
a pair list may take, and the scratch it shares with the pair calls."""
import ctypes as C

import numpy as np
import pytest

import bootstrap_shapes as BS
from bootstrap_shapes import CLOSE, MODES, TOL
from pyaudiolocalization_amd import _ffi
from pyaudiolocalization_amd import bootstrap as B
from pyaudiolocalization_amd.engine import make_params, pair_list

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module", autouse=True)
def _engine(engine):
    import pyaudiolocalization_amd.engine as E
    E._default = engine
    yield
    E._default = None


def _source(L):
    return np.arange(L) + 0.5           # a wrong index is readable


def _shuffle(engine, row, i, j, mode, bs, seed, s0, S):
    """shuffles s0 .. s0+S-1 of row -> [S][L]; the buffer is one row longer and must keep its sentinel there"""
    L = row.shape[0]
    d_row, d_out = engine.alloc(row.nbytes), engine.alloc((S + 1) * row.nbytes)
    try:
        engine.upload(d_row, row)
        engine.upload(d_out, np.full((S + 1, L), SENTINEL))
        engine.bootstrap_shuffle_dev(d_row, L, i, j, mode, bs, seed, s0, S, d_out)
        engine.synchronize()
        got = engine.download(np.empty((S + 1, L)), d_out)
    finally:
        engine.free(d_out)
        engine.free(d_row)
    assert np.all(got[S] == SENTINEL), "a store behind the last row"
    return got[:S]


# ---- the shuffle kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", BS.TILING_LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_shuffle_tiling(engine, L, mode):
    i, j, seed = BS.SHUFFLE_KEY
    row, S, bs = _source(L), 5, 3
    got = _shuffle(engine, row, i, j, mode, bs, seed, 0, S)
    for s in range(S):
        assert np.array_equal(got[s], row[B.shuffle_indices(L, i, j, s, mode, bs, seed)]), (mode, L, s)


@pytest.mark.parametrize("L,bs", [(L, bs) for L in BS.BLOCK_LENGTHS for bs in BS.device_block_sizes(L)])
def test_block_mode_degenerate_sizes(engine, L, bs):
    i, j, seed = BS.SHUFFLE_KEY
    row, S = _source(L), BS.BLOCK_SHUFFLES
    want = np.stack([row[B.shuffle_indices(L, i, j, s, "block", bs, seed)] for s in range(S)])
    if (L, bs) == (1000, 50):           # the 'short' last block (full here) lands first in one shuffle and last in another
        assert want[BS.SHORT_BLOCK_FIRST][0] == row[L - bs] and want[BS.SHORT_BLOCK_LAST][L - bs] == row[L - bs]
    if bs >= L:
        assert np.array_equal(want, np.tile(row, (S, 1)))
    got = _shuffle(engine, row, i, j, "block", bs, seed, 0, S)
    for s in range(S):
        assert np.array_equal(got[s], want[s]), (L, bs, s)


@pytest.mark.parametrize("mode,bs", [("permutation", 50), ("block", 2)])
def test_more_rows_than_one_launch(engine, mode, bs):
    """65 536 rows per launch: the next launch starts at shuffle s0 + 65 536 and at row 65 536 of the output"""
    i, j, seed = BS.SHUFFLE_KEY
    L, S, s0 = 5, BS.ROWS_PER_LAUNCH + 3, 11
    row = _source(L)
    got = _shuffle(engine, row, i, j, mode, bs, seed, s0, S)
    assert np.array_equal(np.sort(got, axis=1), np.tile(row, (S, 1)))          # every row is a permutation of the source
    for k in (0, 1, 65534, 65535, 65536, 65537, 65538):
        assert np.array_equal(got[k], row[B.shuffle_indices(L, i, j, s0 + k, mode, bs, seed)]), (mode, k)
    if mode == "permutation":                                                    # (not one shuffle repeated)
        assert len({r.tobytes() for r in got[65530:65539]}) > 3


@pytest.mark.parametrize("i,j,s0,seed", BS.WIDE_KEYS)
@pytest.mark.parametrize("mode", MODES)
def test_wide_counters(engine, mode, i, j, s0, seed):
    L, S, bs = 1025, 3, 47
    row = _source(L)
    got = _shuffle(engine, row, i, j, mode, bs, seed, s0, S)
    for k in range(S):
        assert np.array_equal(got[k], row[B.shuffle_indices(L, i, j, s0 + k, mode, bs, seed)]), (mode, k)


def test_shuffle_refusals_leave_the_engine_usable(engine):
    L, S = 1025, 2
    row = _source(L)
    i, j, seed = BS.SHUFFLE_KEY
    d_row, d_out = engine.alloc(row.nbytes), engine.alloc(S * row.nbytes)

    def call(d_src, length, ci, cj, s0, d_dst):
        return engine._lib.pal_bootstrap_shuffle_dev(engine._h, C.c_void_p(d_src), length, ci, cj, _ffi.BOOT_PERMUTATION, 50,
                                                     C.c_uint64(seed), s0, S, C.c_void_p(d_dst))

    try:
        engine.upload(d_row, row)
        for args, want in (((d_row, L, i, j, -1, d_out), _ffi.ERR_INVALID),
                           ((d_row, L, -1, j, 0, d_out), _ffi.ERR_INVALID),
                           ((d_row, L, i, -1, 0, d_out), _ffi.ERR_INVALID),
                           ((d_row, (1 << 20) + 1, i, j, 0, d_out), _ffi.ERR_UNSUPPORTED),
                           ((None, L, i, j, 0, d_out), _ffi.ERR_INVALID),
                           ((d_row, L, i, j, 0, None), _ffi.ERR_INVALID)):
            engine.upload(d_out, np.full((S, L), SENTINEL))
            assert call(*args) == want, args
            engine.synchronize()
            assert np.all(engine.download(np.empty((S, L)), d_out) == SENTINEL), args      # a refused call writes nothing
            assert call(d_row, L, i, j, 0, d_out) == 0
            engine.synchronize()
            got = engine.download(np.empty((S, L)), d_out)
            for s in range(S):
                assert np.array_equal(got[s], row[B.shuffle_indices(L, i, j, s, "permutation", 50, seed)]), (args, s)
    finally:
        engine.free(d_out)
        engine.free(d_row)


# ---- the peaks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 2, 3, 8))
@pytest.mark.parametrize("mode", MODES)
def test_peaks_of_tiny_frames(engine, L, mode):
    rows, pairs, S, bs = BS.frame(3, L), pair_list(3), 4, 2
    got = engine.bootstrap_peaks(rows, pairs, S, mode, bs, seed=5)
    assert got.shape == (3, S)
    assert np.allclose(got, BS.oracle_peaks(rows, pairs, S, mode, bs, 5), equal_nan=True, **TOL)


@pytest.mark.parametrize("L,n1,n2,tile", BS.ROUTES)
def test_peaks_on_every_route(engine, L, n1, n2, tile):
    """seven shuffled rows per pair list of three: 21 rows in one odd round, the last transform half empty; their spectra lie behind
    the three original rows' in whatever layout the plan gives a spectrum row"""
    info = engine.plan_info(L)
    assert (info["n1"], info["n2"], info["tile_len"]) == (n1, n2, tile), info
    rows, pairs, S = BS.frame(3, L), pair_list(3), 7
    got = engine.bootstrap_peaks(rows, pairs, S, "block", 50, seed=6)
    assert np.allclose(got, BS.oracle_peaks(rows, pairs, S, "block", 50, 6), **TOL)


def _peaks_dev(engine, rows, pairs, S, mode, bs, seed):
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    R, L = rows.shape
    d_rows, d_pairs, d_peaks = engine.alloc(rows.nbytes), engine.alloc(pairs.nbytes), engine.alloc(len(pairs) * S * 8)
    try:
        engine.upload(d_rows, rows)
        engine.upload(d_pairs, pairs)
        engine.bootstrap_peaks_dev(d_rows, R, L, d_pairs, len(pairs), S, mode, bs, seed, d_peaks)
        engine.synchronize()
        return engine.download(np.empty((len(pairs), S)), d_peaks)
    finally:
        engine.free(d_peaks)
        engine.free(d_pairs)
        engine.free(d_rows)


def test_round_boundary_at_the_default_group_size(engine):
    """bootstrap_round's first outcome, four whole launch groups: 2000 shuffles of one pair are 1920 rows and 80"""
    L, S, seed = 600, 2000, 12
    assert 4 * 2 * engine.pair_group_size(L) == 1920
    rows = BS.frame(2, L)
    one = engine.bootstrap_peaks(rows, [[0, 1]], S, "permutation", 50, seed)
    want = BS.oracle_peaks(rows, [(0, 1)], S, "permutation", 50, seed, BS.BOUNDARY_SHUFFLES)
    assert np.allclose(one[:, list(BS.BOUNDARY_SHUFFLES)], want, **TOL)
    assert _peaks_dev(engine, rows, [[0, 1]], S, "permutation", 50, seed).tobytes() == one.tobytes()
    # keyed per pair, not per round: the second pair's shuffles 920 .. 999 fall into the second round
    two = engine.bootstrap_peaks(rows, [[0, 1], [1, 0]], 1000, "permutation", 50, seed)
    assert np.allclose(two[0], one[0, :1000], **CLOSE)
    at = (0, 919, 920, 999)
    assert np.allclose(two[1, list(at)], BS.oracle_peaks(rows, [(1, 0)], 1000, "permutation", 50, seed, at)[0], **TOL)


def test_round_boundary_in_whole_groups_under_the_cap(engine):
    """bootstrap_round's second outcome: at L = 44 100 the 1 GiB cap holds two launch groups and a bit, rounded down to whole groups
    (a shuffled row takes 8 L bytes and its spectrum 16 bytes per bin of the 89 x 991 plan's 45 rows of 991).  1000 shuffles of one
    pair cross into a second round."""
    L, S, seed = 44100, 1000, 14
    info = engine.plan_info(L)
    assert (info["n1"], info["n2"]) == (89, 991), info
    group = 2 * engine.pair_group_size(L)
    cap = 2**30 // (8 * L + 16 * 45 * 991)
    assert 2 * group <= cap < 3 * group and 2 * group < S
    rows = BS.frame(2, L)
    got = engine.bootstrap_peaks(rows, [[0, 1]], S, "permutation", 50, seed)
    at = (0, group - 1, group, 2 * group - 2, 2 * group - 1, 2 * group, 2 * group + 1, S - 1)
    assert np.allclose(got[0, list(at)], BS.oracle_peaks(rows, [(0, 1)], S, "permutation", 50, seed, at)[0], **TOL)


def test_long_rows_round_below_one_launch_group(engine):
    """bootstrap_round's third outcome: the 1 GiB cap holds fewer rows than one launch group, so the round is the cap itself, an
    odd number of rows that is a multiple of nothing.  A shuffled row and its spectrum take at least 24 L bytes (a spectrum row holds
    at least the L non-redundant bins), which bounds the round from above without naming it."""
    L, S, seed = BS.LONG_L, BS.LONG_S, 31
    most = 2**30 // (24 * L)
    assert most < 2 * engine.pair_group_size(L) and 2 * most < S          # below one launch group; at least three rounds
    rows = BS.frame(2, L)
    got = engine.bootstrap_peaks(rows, [[0, 1]], S, "permutation", 50, seed)[0]
    # second witness: the same shuffled rows, built on the device behind the fixed row, through the pair pipeline
    pairs = np.stack([np.zeros(S, np.int32), np.arange(1, S + 1, dtype=np.int32)], axis=1)
    table = np.zeros(S, dtype=_ffi.RECORD)
    d_src, d_all = engine.alloc(L * 8), engine.alloc((S + 1) * L * 8)
    d_pairs, d_table = engine.alloc(pairs.nbytes), engine.alloc(table.nbytes)
    try:
        engine.upload(d_src, rows[1])
        engine.upload(d_all, rows[0])
        engine.upload(d_pairs, pairs)
        engine.bootstrap_shuffle_dev(d_src, L, 0, 1, "permutation", 50, seed, 0, S, d_all + L * 8)
        engine.gcc_phat_pairs_dev(d_all, S + 1, L, d_pairs, S, make_params(1000.0), d_table)
        engine.synchronize()
        engine.download(table.view(np.uint8), d_table)
    finally:
        for d in (d_table, d_pairs, d_all, d_src):
            engine.free(d)
    assert np.allclose(got, table["cmax"], **CLOSE)
    at = list(BS.LONG_ORACLE_SHUFFLES)
    assert len(at) == 26 and at[0] == 0 and at[-1] == S - 1
    assert np.allclose(got[at], BS.oracle_peaks(rows, [(0, 1)], S, "permutation", 50, seed, at)[0], **TOL)


def test_pair_list_forms(engine):
    rows, S = BS.frame(4, 600), 6
    pairs = np.array(BS.PAIR_FORMS, dtype=np.int32)
    got = engine.bootstrap_peaks(rows, pairs, S, "block", 50, seed=9)
    assert np.allclose(got, BS.oracle_peaks(rows, pairs, S, "block", 50, 9), **TOL)      # per row of the list
    assert np.allclose(got[2], got[3], **CLOSE)                  # (1, 2) twice
    assert not np.allclose(got[1], got[2], **CLOSE)              # (2, 1) is another pair: the key is ordered
    lone = engine.bootstrap_peaks(rows[:1], [[0, 0]], S, "block", 50, seed=9)
    assert np.allclose(lone, BS.oracle_peaks(rows[:1], [(0, 0)], S, "block", 50, 9), **TOL)


def test_nothing_left_behind_in_shared_scratch(engine):
    """the bootstrap keeps its spectra in the slot the pair calls use: neither leaves anything the other one reads"""
    from pyaudiolocalization_amd import Engine
    rows, pairs = BS.frame(3, 600), pair_list(3)
    frames = BS.frame(4, 2500)
    first = engine.bootstrap_peaks(rows, pairs, 40, "circular", 50, seed=2)
    table = engine.gcc_phat_all_pairs(frames, 16000.0)
    again = engine.bootstrap_peaks(rows, pairs, 40, "circular", 50, seed=2)
    assert again.tobytes() == first.tobytes()
    assert np.allclose(first, BS.oracle_peaks(rows, pairs, 40, "circular", 50, 2), **TOL)
    fresh = Engine(engine.device)
    try:
        want = fresh.gcc_phat_all_pairs(frames, 16000.0)
    finally:
        fresh.close()
    assert table.tobytes() == want.tobytes()
