"""The loop-closure check on the device (pal_tdoa_closure*, csrc/closure.hip) against its specification (closure.py), byte for byte:
shapes around the vote kernel's tile edge T = 16 (one workgroup per 16 x 16 tile of pairs: M = 16, 17 and 33 are T, T + 1 and 2 T + 1),
batches, parameters, NULL outputs, extreme lags, errors; then the solve under ``weights='closure'``, the stream, and no state left behind."""
import ctypes as C_
import itertools

import numpy as np
import pytest

import closure_tables as CT
import robust_tables as T
from oracle import cases
from pyaudiolocalization_amd import _ffi
from pyaudiolocalization_amd import closure as CL
from pyaudiolocalization_amd import solve as S

pytestmark = pytest.mark.gpu

FIVE_LENGTHS = np.array([24000, 3000, 1, 65536, 12345], dtype=np.int64)
KW = dict(buffer=T.BUFFER, grid=T.GRID)


def _frames(m, b, lengths):
    """k_sel[b][P]: frame 0 an outlier table of robust_tables (a quarter of the pairs replaced), the others random lags that
    close some triangles; each frame on its own length (lags clipped to what the length allows)."""
    p = m * (m - 1) // 2
    lag = CT.random_tables(b, m, 21, span=4) - (T.LENGTH - 1)
    lag[0] = T.table(m, 5, p // 4)["lag"]
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (b,))
    lag = np.clip(lag, -(ln[:, None] - 1), ln[:, None] - 1)
    return lag + ln[:, None] - 1, ln


def _dev(engine, k_sel, lengths, m, tol=1, min_votes=1, mode="soft", outputs=CL.OUTPUTS, sync=True):
    """Engine.tdoa_closure_dev around device buffers -> the four outputs (None where not asked for)."""
    tab = CT.records(np.atleast_2d(k_sel))
    out = CL.empty_outputs(tab.shape[0], m, outputs)
    d_tab = engine.alloc(tab.nbytes)
    d_out = [engine.alloc(a.nbytes) if a is not None else 0 for a in out]
    try:
        engine.upload(d_tab, tab)
        engine.tdoa_closure_dev(d_tab, tab.shape[0], m, lengths, tol, min_votes, mode, *d_out)
        if sync:
            engine.synchronize()
        for a, d in zip(out, d_out):
            if a is not None:
                engine.download(a, d)
    finally:
        engine.free(d_tab)
        for d in d_out:
            if d:
                engine.free(d)
    return out


def _host(engine, k_sel, lengths, m, tol=1, min_votes=1, mode="soft", outputs=CL.OUTPUTS):
    return engine.tdoa_closure(CT.records(np.atleast_2d(k_sel)), lengths, m, tol, min_votes, mode, outputs=outputs)


def _assert_same(got, want, what):
    for name, g, w in zip(CL.OUTPUTS, got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("m", [3, 4, 16, 17, 33, 65])
def test_shapes_batches_and_parameters(engine, m):
    for b, lengths in ((1, T.LENGTH), (5, FIVE_LENGTHS)):
        k_sel, ln = _frames(m, b, lengths)
        for tol in (0, 1, 5):
            for min_votes in (0, 1, m - 2, m - 1):
                for mode in ("mask", "soft"):
                    want = CT.spec(k_sel, ln, m, tol, min_votes, mode)
                    _assert_same(_dev(engine, k_sel, ln, m, tol, min_votes, mode), want, ("dev", b, tol, min_votes, mode))
                    _assert_same(_host(engine, k_sel, ln, m, tol, min_votes, mode), want, ("host", b, tol, min_votes, mode))
        if b == 1:
            want = CT.spec(k_sel, ln, m, 1, 1, "soft")
            print(f"[closure] M = {m}: votes {want[0].min()}..{want[0].max()}, {want[3][0]['closed']} of {want[3][0]['triangles']} triangles closed, "
                  f"{want[3][0]['kept_pairs']} pairs kept")
            assert 0 < want[3][0]["closed"] or m == 3                                           # the inputs exercise both answers
    k_sel, ln = _frames(m, 5, FIVE_LENGTHS)
    assert np.all(CT.spec(k_sel, ln, m, 1, m - 1, "soft")[2] == 0)                              # min_votes above M - 2: valid, all-zero weights


def test_256_microphones(engine):
    t = T.table(256, 9, 3000)
    for tol, min_votes, mode in ((1, 1, "soft"), (0, 254, "mask")):
        want = CT.spec(t["k_sel"], T.LENGTH, 256, tol, min_votes, mode)
        _assert_same(_dev(engine, t["k_sel"], T.LENGTH, 256, tol, min_votes, mode), want, ("dev", tol))
        _assert_same(_host(engine, t["k_sel"], T.LENGTH, 256, tol, min_votes, mode), want, ("host", tol))
    s = CT.spec(t["k_sel"], T.LENGTH, 256, 1, 1, "soft")[3][0]
    print(f"[closure] M = 256, 3000 replaced pairs: {s['closed']} of {s['triangles']} triangles closed, {s['kept_pairs']} of 32640 pairs kept")
    assert s["triangles"] == 2763520 and 0 < s["closed"] < s["triangles"]


def test_every_subset_of_outputs(engine):
    k_sel, ln = _frames(17, 3, FIVE_LENGTHS[:3])
    want = CT.spec(k_sel, ln, 17, 1, 2, "soft")
    for r in range(1, 5):
        for outputs in itertools.combinations(CL.OUTPUTS, r):
            for form in (_dev, _host):
                got = form(engine, k_sel, ln, 17, 1, 2, "soft", outputs=outputs)
                assert [g is not None for g in got] == [name in outputs for name in CL.OUTPUTS]
                _assert_same(got, want, (form.__name__, outputs))


def test_a_frame_alone_and_in_a_batch_of_eight(engine):
    k_sel, ln = _frames(33, 8, np.array([24000, 3000, 500, 65536, 12345, 24000, 777, 4096]))
    batch = _dev(engine, k_sel, ln, 33, 1, 1, "soft")
    _assert_same(batch, CT.spec(k_sel, ln, 33, 1, 1, "soft"), "batch")
    for f in range(8):
        alone = _dev(engine, k_sel[f], ln[f:f + 1], 33, 1, 1, "soft")
        for name, a, full in zip(CL.OUTPUTS, alone, batch):
            assert a[0].tobytes() == full[f].tobytes(), (f, name)


def test_extreme_lags(engine):
    length = 1 << 19
    k_sel = np.array([[(0, 2 * length - 2)[bit] for bit in bits] for bits in itertools.product((0, 1), repeat=3)], dtype=np.int64)
    for tol in (0, 1 << 20):
        want = CT.spec(k_sel, length, 3, tol, 1, "soft")
        _assert_same(_dev(engine, k_sel, length, 3, tol), want, ("dev", tol))
        _assert_same(_host(engine, k_sel, length, 3, tol), want, ("host", tol))
    sums = np.array([abs((a - b + c) * (length - 1)) for a, b, c in itertools.product((-1, 1), repeat=3)])      # xy + yz - xz
    assert np.array_equal(CT.spec(k_sel, length, 3, 1 << 20, 1, "soft")[3]["closed"], (sums <= 1 << 20).astype(np.int32))
    assert sums.max() == 3 * (length - 1)                                                       # all three sides add up in two of the eight


def _raw(engine, symbol, tab, b, m, lengths, tol, min_votes, mode, outputs=True):
    """The C ABI itself (host form: tab a record array; _dev form: tab a device pointer) -> return code."""
    ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.int32), (max(b, 1),)))
    p = max(m * (m - 1) // 2, 1)
    host = symbol == "pal_tdoa_closure"
    votes = np.zeros((max(b, 1), p), dtype=np.int32)
    d_votes = 0
    if outputs and not host:
        d_votes = engine.alloc(votes.nbytes)
    try:
        out = [votes.ctypes.data if host else C_.c_void_p(d_votes), None, None, None] if outputs else [None] * 4
        return getattr(engine._lib, symbol)(engine._h, tab.ctypes.data if host else C_.c_void_p(tab), b, m, ln.ctypes.data, tol, min_votes, mode, *out)
    finally:
        if d_votes:
            engine.free(d_votes)


def _works(engine):
    k_sel, ln = _frames(17, 2, FIVE_LENGTHS[:2])
    want = CT.spec(k_sel, ln, 17, 1, 1, "soft")
    _assert_same(_dev(engine, k_sel, ln, 17), want, "dev after an error")
    _assert_same(_host(engine, k_sel, ln, 17), want, "host after an error")


def test_errors_and_the_call_after(engine):
    t = T.table(4, 5, 1)
    tab = t["records"][None].copy()
    d_tab = engine.alloc(tab.nbytes)
    try:
        engine.upload(d_tab, tab)
        bad_args = [dict(m=2), dict(m=257), dict(tol=-1), dict(tol=(1 << 20) + 1), dict(b=0), dict(min_votes=-1), dict(mode=2), dict(mode=-1),
                    dict(lengths=0), dict(lengths=(1 << 24) + 1), dict(outputs=False)]
        for change in bad_args:
            for symbol, table in (("pal_tdoa_closure", tab), ("pal_tdoa_closure_dev", d_tab)):
                args = {**dict(b=1, m=4, lengths=T.LENGTH, tol=1, min_votes=1, mode=1), **change}
                assert _raw(engine, symbol, table, **args) == _ffi.ERR_INVALID, (symbol, change)
                engine.synchronize()                                                            # nothing was enqueued, nothing is pending
            _works(engine)
        assert _raw(engine, "pal_tdoa_closure", tab, 1, 4, T.LENGTH, 1, 7, 1) == 0              # min_votes above M - 2 is valid
    finally:
        engine.free(d_tab)
    for kw in (dict(m=2), dict(tol=-1), dict(mode="hard"), dict(min_votes=-1), dict(lengths=0)):
        with pytest.raises(ValueError):
            engine.tdoa_closure(**{**dict(tables=t["records"], lengths=T.LENGTH, m=4), **kw})
        with pytest.raises(ValueError):
            engine.tdoa_closure_dev(**{**dict(d_tables=0, b=1, m=4, lengths=T.LENGTH, d_votes=0), **kw})
    for bad_k in (2 * T.LENGTH - 1, -1):
        k_sel = np.stack([t["k_sel"], t["k_sel"]])
        k_sel[1, 3] = bad_k
        with pytest.raises(ValueError):
            _host(engine, k_sel, T.LENGTH, 4)
        _works(engine)
        with pytest.raises(ValueError) as err:                                                  # enqueued without complaint, reported by synchronize
            _dev(engine, k_sel, T.LENGTH, 4)
        assert "k_sel" in str(err.value)
        engine.synchronize()                                                                    # reported once
        _works(engine)
    k_sel = t["k_sel"].copy()
    k_sel[0] = 2 * T.LENGTH - 2                                                                 # the last valid index
    _assert_same(_dev(engine, k_sel, T.LENGTH, 4), CT.spec(k_sel, T.LENGTH, 4), "edge")


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", T.OUTLIER_CASES)
def test_solve_with_closure_weights(engine, case):
    from pyaudiolocalization_amd.main import solve_positions_device
    t = T.table(*case)
    m = case[0]
    tabs = np.stack([t["records"], T.table(m, case[1], 0)["records"]])                          # the outlier table and its clean one
    k_sel = np.stack([t["k_sel"], T.table(m, case[1], 0)["k_sel"]])
    for kw in (dict(), dict(closure_tol=2, closure_min_votes=2, closure_mode="mask")):
        spec_kw = dict(tol=kw.get("closure_tol", 1), min_votes=kw.get("closure_min_votes", 1), mode=kw.get("closure_mode", "soft"))
        weights = CT.spec(k_sel, T.LENGTH, m, **spec_kw)[2]
        want = engine.solve_positions(tabs, T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights=weights, **KW)
        got = engine.solve_positions(tabs, T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", **KW, **kw)
        assert got.tobytes() == want.tobytes(), (case, kw, "host form")
        d_tab = engine.alloc(tabs.nbytes)
        try:
            engine.upload(d_tab, tabs)
            dev = engine.solve_positions_dev(d_tab, 2, T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", **KW, **kw)
        finally:
            engine.free(d_tab)
        assert dev.tobytes() == want.tobytes(), (case, kw, "_dev form")
        pos = solve_positions_device(tabs, T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", engine=engine, **KW, **kw)
        assert np.array_equal(pos, want["position"])
        dist = np.linalg.norm(want["position"] - T.SRC, axis=1)
        print(f"[closure] {case} {spec_kw}: {dist[0]:.4f} m from the source with {t['bad'].size} replaced pairs, {dist[1]:.4f} m on the clean table")
        if not kw:                                                                              # the default: tol 1, one vote, soft
            assert np.all(want["status"] & S.ST_CONVERGED)
            assert dist[0] < 0.15 and dist[1] < 0.15, case
    with pytest.raises(ValueError):
        engine.solve_positions(tabs, T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="votes", **KW)


def test_position_stream_with_closure_weights(engine):
    from pyaudiolocalization_amd.stream import position_stream, tdoa_stream
    from test_gpu_stream import _c5_like_frames
    bases, delays, gains, totals, trim, fs = _c5_like_frames(7)
    pos = np.random.default_rng(55).uniform(-0.4, 0.4, (8, 3))           # the array of _c5_like_frames
    c = cases.C_SOUND
    tables, lengths = tdoa_stream(bases, delays, gains, fs, totals, trim, "butterworth", 0.05, engine=engine, frames_per_batch=4)
    p2, t2, l2 = position_stream(bases, delays, gains, fs, totals, trim, pos, c, "butterworth", 0.05, engine=engine, frames_per_batch=4,
                                 weights="closure", closure_tol=2)
    assert t2.tobytes() == tables.tobytes() and np.array_equal(l2, lengths)
    assert p2.tobytes() == engine.solve_positions(tables, lengths, pos, fs, c, weights="closure", closure_tol=2).tobytes()
    weights = CT.spec(tables["k_sel"], lengths, 8, 2, 1, "soft")[2]
    assert p2.tobytes() == engine.solve_positions(tables, lengths, pos, fs, c, weights=weights).tobytes()


def test_no_state_left_behind(engine):
    t = T.table(16, 3, 30)
    before = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="ones", **KW)
    engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="closure", **KW)
    _host(engine, t["k_sel"], T.LENGTH, 16)
    after = engine.solve_positions(t["records"], T.LENGTH, t["mics"], T.FS, T.C_SOUND, weights="ones", **KW)
    assert after.tobytes() == before.tobytes()
