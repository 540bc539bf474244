"""The loop-closure consensus on the device (pal_tdoa_consensus*, csrc/consensus.hip) against its specification (consensus.py), byte for
byte: shapes around the tile edge T = 16 of the pair kernels (M = 16, 17 and 33 are T, T + 1 and 2 T + 1), every cube width (K = 1, 2, 4, 8)
with rows that hold fewer candidates, batches on five lengths, tolerances, rounds, NULL outputs, extreme lags, one 256-microphone frame
through the chunked-LDS path, errors; then table_out through the closure check and the solve, and no state left behind (the chain from
simulated frames: tests/test_gpu_pairs_peaks.py)."""
import ctypes as C_
import itertools

import numpy as np
import pytest

import closure_tables as CT
import consensus_tables as CS
import robust_tables as T
from pyaudiolocalization_amd import _ffi
from pyaudiolocalization_amd import consensus as CN

pytestmark = pytest.mark.gpu

FIVE_LENGTHS = np.array([24000, 3000, 1, 65536, 12345], dtype=np.int64)
KW = dict(buffer=T.BUFFER, grid=T.GRID)


def _frames(m, k, b, lengths):
    """cand_k[b][P][k] (int64) with trailing candidates removed at random, each frame on its own length (lags clipped to what the
    length allows), tables[b][P] whose every field is set, cand_h[b][P][k]."""
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (b,))
    lag = np.stack([CS.random_candidates(m, 21 + f, .5, k, .1)["cand_k"] for f in range(b)]) - (T.LENGTH - 1)
    lag = np.clip(lag, -(ln[:, None, None] - 1), ln[:, None, None] - 1)
    cand = CS.ragged(lag + ln[:, None, None] - 1, m)
    rng = np.random.default_rng([m, k, b])
    tab = CT.records(cand[..., 0])
    tab["branch"] = rng.integers(0, 16, tab.shape)
    tab["k_argmax"] = cand[..., 0]
    tab["n_sel"] = np.count_nonzero(cand != CN.ABSENT, axis=2)
    for name in ("cmax", "cmin", "snr", "sel_height"):
        tab[name] = rng.standard_normal(tab.shape)
    heights = np.where(cand != CN.ABSENT, rng.standard_normal(cand.shape), 0.0)
    return cand, ln, tab, heights


def _want(cand, ln, m, tol, rounds, tab=None, heights=None):
    sel, summary = CS.spec(cand, ln, m, tol, rounds)
    return sel, None if tab is None else CN.apply(tab, cand, heights, sel), summary


def _dev(engine, cand, ln, m, tol=1, rounds=2, tab=None, heights=None, outputs=CN.OUTPUTS, sync=True):
    """Engine.tdoa_consensus_dev around device buffers -> the three outputs (None where not asked for)."""
    ck = np.ascontiguousarray(cand, dtype=np.int32)
    ck = ck[None] if ck.ndim == 2 else ck
    b, p, k = ck.shape
    out = [np.zeros((b, p), dtype=np.int32), np.zeros((b, p), dtype=_ffi.RECORD), np.zeros(b, dtype=CN.SUMMARY)]
    out = [a if name in outputs else None for name, a in zip(CN.OUTPUTS, out)]
    inputs = [ck, None if tab is None else np.ascontiguousarray(tab), None if heights is None else np.ascontiguousarray(heights, dtype=np.float64)]
    d_in = [engine.alloc(a.nbytes) if a is not None else 0 for a in inputs]
    d_out = [engine.alloc(a.nbytes) if a is not None else 0 for a in out]
    try:
        for a, d in zip(inputs, d_in):
            if a is not None:
                engine.upload(d, a)
        engine.tdoa_consensus_dev(d_in[0], b, m, k, ln, tol, rounds, d_tables=d_in[1], d_cand_h=d_in[2], d_sel=d_out[0], d_table_out=d_out[1],
                                  d_summary=d_out[2])
        if sync:
            engine.synchronize()
        for a, d in zip(out, d_out):
            if a is not None:
                engine.download(a, d)
    finally:
        for d in d_in + d_out:
            if d:
                engine.free(d)
    return out


def _host(engine, cand, ln, m, tol=1, rounds=2, tab=None, heights=None, outputs=CN.OUTPUTS):
    return engine.tdoa_consensus(cand, ln, m, tol, rounds, tables=tab, cand_h=heights, outputs=outputs)


def _assert_same(got, want, what):
    for name, g, w in zip(CN.OUTPUTS, got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("m", [3, 4, 16, 17, 33, 65])
def test_shapes_batches_and_parameters(engine, m):
    every = list(itertools.product((0, 1, 5), (0, 1, 4)))                                    # (tol, rounds)
    some = [(1, 1), (0, 4), (5, 0)]

    def combos(k, b):
        """Every combination on the small arrays; on the larger ones as many as keep the specification's stage 0 (P M K^3) at seconds."""
        if m <= 17 or (k == 4 and b == 1):
            return every
        if k == 8 and b == 5:
            return [(1, 1)]
        return some
    for k in (1, 2, 4, 8):
        for b, lengths in ((1, T.LENGTH), (5, FIVE_LENGTHS)):
            cand, ln, tab, heights = _frames(m, k, b, lengths)
            assert k == 1 or np.any(cand == CN.ABSENT)
            for tol, rounds in combos(k, b):
                want = _want(cand, ln, m, tol, rounds, tab, heights)
                _assert_same(_dev(engine, cand, ln, m, tol, rounds, tab, heights), want, ("dev", k, b, tol, rounds))
                _assert_same(_host(engine, cand, ln, m, tol, rounds, tab, heights), want, ("host", k, b, tol, rounds))
            if b == 1 and k == 4:
                s = CS.spec(cand, ln, m, 1, 4)[1][0]
                print(f"[consensus] M = {m}, K = 4: {s['moved']} pairs moved, closed triangles {s['closed_before']} -> {s['closed_after']}, "
                      f"{s['changed_last']} changed in round 4")
                assert m < 8 or s["closed_after"] > s["closed_before"]                      # the inputs give the rule something to do


def test_256_microphones_through_the_chunked_path(engine):
    cand = CS.big_frame()
    for rounds in (0, 2):
        want = CS.big_spec(rounds)
        got = _dev(engine, cand, np.array([T.LENGTH]), 256, CS.BIG["tol"], rounds, outputs=("sel", "summary"))
        _assert_same(got, (want[0], None, want[1]), ("dev", rounds))
    got = _host(engine, cand, T.LENGTH, 256, CS.BIG["tol"], 2, outputs=("sel", "summary"))
    _assert_same(got, (want[0], None, want[1]), "host")
    s = want[1][0]
    print(f"[consensus] M = 256, K = 8: {s['moved']} of 32640 pairs moved, closed triangles {s['closed_before']} -> {s['closed_after']}")


def test_every_subset_of_outputs_and_optional_inputs(engine):
    cand, ln, tab, heights = _frames(17, 4, 3, FIVE_LENGTHS[:3])
    want = _want(cand, ln, 17, 1, 2, tab, heights)
    for r in range(1, 4):
        for outputs in itertools.combinations(CN.OUTPUTS, r):
            for form in (_dev, _host):
                got = form(engine, cand, ln, 17, 1, 2, tab, heights, outputs=outputs)
                assert [g is not None for g in got] == [name in outputs for name in CN.OUTPUTS]
                _assert_same(got, want, (form.__name__, outputs))
    no_heights = _want(cand, ln, 17, 1, 2, tab, None)                                        # sel_height is then copied
    assert np.array_equal(no_heights[1]["sel_height"], tab["sel_height"])
    for form in (_dev, _host):
        _assert_same(form(engine, cand, ln, 17, 1, 2, tab, None), no_heights, (form.__name__, "no heights"))
        _assert_same(form(engine, cand, ln, 17, 1, 2, None, None, outputs=("sel", "summary")), want, (form.__name__, "no tables"))


def test_the_summary_votes_are_closure_launches(engine):
    """A call with a summary takes the closure votes of candidate 0 and of the result from k_closure_votes (two launches) and runs
    k_consensus_round exactly ``rounds`` times; a call without one launches no k_closure_votes."""
    cand, ln, tab, heights = _frames(17, 2, 2, FIVE_LENGTHS[:2])
    want = _want(cand, ln, 17, 1, 2, tab, heights)
    for outputs, votes_launches in ((CN.OUTPUTS, 2), (("sel", "table_out"), 0)):
        engine.profile_begin()
        got = _dev(engine, cand, ln, 17, 1, 2, tab, heights, outputs=outputs)
        engine.profile_end()
        launches = {name: v[1] for name, v in engine.profile_entries().items()}
        assert launches.get("k_closure_votes", 0) == votes_launches, (outputs, launches)
        assert launches.get("k_consensus_round", 0) == 2, (outputs, launches)
        _assert_same(got, want, outputs)


def test_a_frame_alone_and_in_a_batch(engine):
    cand, ln, tab, heights = _frames(33, 4, 5, FIVE_LENGTHS)
    batch = _dev(engine, cand, ln, 33, 1, 2, tab, heights)
    _assert_same(batch, _want(cand, ln, 33, 1, 2, tab, heights), "batch")
    for f in range(5):
        alone = _dev(engine, cand[f], ln[f:f + 1], 33, 1, 2, tab[f:f + 1], heights[f:f + 1])
        for name, a, full in zip(CN.OUTPUTS, alone, batch):
            assert a[0].tobytes() == full[f].tobytes(), (f, name)


def test_extreme_lags(engine):
    length = 1 << 24
    orders = list(itertools.permutations((0, length - 1, 2 * length - 2), 2))               # two of the lags -(L - 1), 0, L - 1 in either order
    cand = np.array([[orders[o] for o in frame] for frame in itertools.product(range(6), repeat=3)], dtype=np.int64)      # [216][3][2]
    for tol in (0, 1 << 20):
        for rounds in (0, 2):
            want = _want(cand, length, 3, tol, rounds)
            _assert_same(_dev(engine, cand, length, 3, tol, rounds, outputs=("sel", "summary")), want, ("dev", tol, rounds))
            _assert_same(_host(engine, cand, length, 3, tol, rounds, outputs=("sel", "summary")), want, ("host", tol, rounds))
    sel, summary = CS.spec(cand, length, 3, 0, 0)
    assert np.any(sel != 0) and np.any(summary["closed_after"] > summary["closed_before"])  # triangles that close only when re-chosen


def test_table_out_through_the_closure_check(engine):
    for cand, ln, m in ((_frames(33, 4, 2, FIVE_LENGTHS[:2])[:2] + (33,)), (CS.big_frame()[None], np.array([T.LENGTH]), 256)):
        tab = CT.records(cand[..., 0])
        sel, table_out, summary = _host(engine, cand, ln, m, 1, 2, tab)
        assert np.array_equal(table_out["k_sel"], np.stack([CN.chosen_k(cand[f], sel[f]) for f in range(cand.shape[0])]))
        assert np.array_equal(table_out["branch"] != 0, sel != 0)
        for tables, name in ((tab, "closed_before"), (table_out, "closed_after")):
            votes = engine.tdoa_closure(tables, ln, m, 1, outputs=("votes",))[0]
            assert np.array_equal(votes.sum(axis=1) // 3, summary[name]), name


def _raw(engine, symbol, bufs, b=1, m=4, k=2, lengths=T.LENGTH, tol=1, rounds=2, outputs=True, cand=True):
    """The C ABI itself (host form: ``bufs`` host arrays; _dev form: device pointers) of (cand_k, sel) -> return code."""
    ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.int32), (max(b, 1),)))
    wrap = (lambda a: a.ctypes.data) if symbol == "pal_tdoa_consensus" else C_.c_void_p
    return getattr(engine._lib, symbol)(engine._h, None, wrap(bufs[0]) if cand else None, None, b, m, k, ln.ctypes.data, tol, rounds,
                                        wrap(bufs[1]) if outputs else None, None, None)


def _works(engine):
    cand, ln, tab, heights = _frames(17, 2, 2, FIVE_LENGTHS[:2])
    want = _want(cand, ln, 17, 1, 1, tab, heights)
    _assert_same(_dev(engine, cand, ln, 17, 1, 1, tab, heights), want, "dev after an error")
    _assert_same(_host(engine, cand, ln, 17, 1, 1, tab, heights), want, "host after an error")


def test_errors_and_the_call_after(engine):
    good = CS.random_candidates(4, 5, .3, 2, 0)["cand_k"]
    host = (np.ascontiguousarray(good, dtype=np.int32), np.zeros(6, dtype=np.int32))
    dev = (engine.alloc(host[0].nbytes), engine.alloc(host[1].nbytes))
    try:
        engine.upload(dev[0], host[0])
        for symbol, bufs in (("pal_tdoa_consensus", host), ("pal_tdoa_consensus_dev", dev)):
            assert _raw(engine, symbol, bufs) == 0
            engine.synchronize()
            for change in (dict(m=2), dict(m=257), dict(k=0), dict(k=9), dict(b=0), dict(tol=-1), dict(tol=(1 << 20) + 1), dict(rounds=-1), dict(rounds=9),
                           dict(lengths=0), dict(lengths=(1 << 24) + 1), dict(outputs=False), dict(cand=False)):
                assert _raw(engine, symbol, bufs, **change) == _ffi.ERR_INVALID, (symbol, change)
                engine.synchronize()                                                        # nothing was enqueued, nothing is pending
            _works(engine)
        rc = engine._lib.pal_tdoa_consensus_dev(engine._h, None, C_.c_void_p(dev[0]), None, 1, 4, 2, np.array([T.LENGTH], dtype=np.int32).ctypes.data,
                                                1, 2, None, C_.c_void_p(dev[1]), None)
        assert rc == _ffi.ERR_INVALID                                                       # table_out without the tables to copy
    finally:
        for d in dev:
            engine.free(d)
    for kw in (dict(m=2), dict(tol=-1), dict(rounds=9), dict(lengths=0), dict(cand_k=good[:, :0]), dict(cand_k=np.zeros((6, 9), dtype=np.int32)),
               dict(outputs=("table_out",)), dict(outputs=("votes",)), dict(outputs=())):
        with pytest.raises(ValueError):
            engine.tdoa_consensus(**{**dict(cand_k=good, lengths=T.LENGTH, m=4), **kw})
    for kw in (dict(m=2), dict(k=0), dict(k=9), dict(tol=-1), dict(rounds=-1), dict(lengths=0)):
        with pytest.raises(ValueError):
            engine.tdoa_consensus_dev(**{**dict(d_cand_k=0, b=1, m=4, k=2, lengths=T.LENGTH, d_sel=0), **kw})
    gap = np.concatenate([good, good[:, :1]], axis=1)
    gap[4, 1] = -1
    for bad, text in (((1, 1, 2 * T.LENGTH - 1), "candidate"), ((5, 0, -2), "candidate"), ((3, 0, -1), "candidate"), (None, "candidate")):
        cand = np.stack([good, good]) if bad is not None else np.stack([gap, gap])
        if bad is not None:
            cand[1][bad[0], bad[1]] = bad[2]
        with pytest.raises(ValueError):
            _host(engine, cand, T.LENGTH, 4, outputs=("sel",))
        _works(engine)
        with pytest.raises(ValueError) as err:                                              # enqueued without complaint, reported by synchronize
            _dev(engine, cand, T.LENGTH, 4, outputs=("sel", "summary"))
        assert text in str(err.value)
        engine.synchronize()                                                                # reported once
        _works(engine)
    edge = good.copy()
    edge[0, 0], edge[2, 1] = 2 * T.LENGTH - 2, -1                                           # the last valid index; an absent last candidate
    _assert_same(_dev(engine, edge, T.LENGTH, 4, outputs=("sel", "summary")), _want(edge, T.LENGTH, 4, 1, 2), "edge")


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CS.TWO_SOURCE_CASES[:2])
def test_solve_on_the_repaired_tables(engine, case):
    from pyaudiolocalization_amd.main import solve_positions_device
    m = case[0]
    t = CS.two_sources(*case)
    cand = t["cand_k"][None]
    tab = CT.records(cand[..., 0])
    heights = np.random.default_rng(case[1]).standard_normal(cand.shape)
    want_tab = _want(cand, T.LENGTH, m, 1, 2, tab, heights)[1]
    first = solve_positions_device(tab, T.LENGTH, t["mics"], T.FS, T.C_SOUND, engine=engine, **KW)
    got = {}
    for name, kw in (("ones", dict()), ("closure", dict(weights="closure"))):
        got[name] = solve_positions_device(tab, T.LENGTH, t["mics"], T.FS, T.C_SOUND, engine=engine, candidates=(cand, heights), **KW, **kw)
        want = solve_positions_device(want_tab, T.LENGTH, t["mics"], T.FS, T.C_SOUND, engine=engine, **KW, **kw)
        assert np.array_equal(got[name], want), (case, kw)
    got = got["ones"]
    one = solve_positions_device(tab[0], T.LENGTH, t["mics"], T.FS, T.C_SOUND, engine=engine, candidates=(cand[0], None), consensus_rounds=2, **KW)
    assert np.array_equal(one, got[0])                                                      # one frame, no heights: the same k_sel
    dist = (np.linalg.norm(first[0] - T.SRC), np.linalg.norm(got[0] - T.SRC))
    print(f"[consensus] {case}: {dist[0]:.4f} m from the source on the first peaks, {dist[1]:.4f} m on the repaired table")
    assert dist[1] < 0.15                                                                   # the bound of the closure tests on clean tables
    with pytest.raises(ValueError):
        solve_positions_device(tab, T.LENGTH, t["mics"], T.FS, T.C_SOUND, engine=engine, candidates=(cand, None), consensus_rounds=9, **KW)


def test_no_state_left_behind(engine):
    t = T.table(16, 3, 30)
    before = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", **KW)
    cand, ln, tab, heights = _frames(16, 8, 2, FIVE_LENGTHS[:2])
    _host(engine, cand, ln, 16, 1, 4, tab, heights)
    _dev(engine, cand, ln, 16, 1, 4, tab, heights)
    after = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", **KW)
    assert after.tobytes() == before.tobytes()
    _assert_same(_dev(engine, cand, ln, 16, 1, 4, tab, heights), _want(cand, ln, 16, 1, 4, tab, heights), "after the solve")
