"""K candidate peaks per pair from the batched GCC-PHAT calls (pal_gcc_phat_all_pairs_peaks[_dev], pal_gcc_phat_pairs_peaks_dev) against the
oracle's selection on the oracle's rows: small frames with odd pair counts (M = 3: a last transform with one pair; M = 5), launch groups of
two transforms so that every call spans several groups and all three streams, the three routes a several-peaks call can take (fused
column pass, prime-factor rows + three statistics launches, four-step + three statistics launches), windowed and unwindowed, both
threshold methods; then the argmax fallbacks, the _dev form, the explicit pair list, the errors and one simulate -> peaks -> consensus ->
solve chain.

Parity rule.  The device's rows equal the oracle's to about 1e-13 (tests/test_gpu_parity.py compares them at that bound on
well-conditioned inputs), and its selection is exact on its own rows; ``test_num_peaks_and_methods`` there relies on no two deciding
heights lying closer than that.  Here a pair is compared only if the oracle's K + 1 highest admissible peaks differ pairwise by more than
MARGIN = 1e-9 (four orders above the rows' difference); the seeds are such that at most a tenth of the pairs of any case is dropped."""
import ctypes as C_
import functools
import itertools

import numpy as np
import pytest

import robust_tables as T
from oracle import cases
from oracle import pal_oracle as O
from pyaudiolocalization_amd import _ffi, make_params, pair_list
from pyaudiolocalization_amd import consensus as CN

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
HEIGHT = dict(rtol=1e-10, atol=1e-13)               # the tolerance of the tests of cmax / sel_height (smoke, test_gpu_parity.py)
FS = 8000.0                                         # peak distance int(fs * 0.001) = 8 samples
K = 4
# the recorded plan table's (tests/golden/plan_table.json) smallest length of each route of a several-peaks call: n = 3 = 1 x 3 (fused
# column pass), n = 16393 = 97 x 169 (N1 > 89: prime-factor rows, three statistics launches), n = 1025 (no split: four-step)
ROUTE_LENGTHS = {"kFused": 2, "kPfa": 8197, "kFourStep": 513}
LENGTHS = [64, 257, 1500] + sorted(ROUTE_LENGTHS.values())
SETTINGS = [(None, "median"), (None, "adaptive"), (0.2, "median"), (0.2, "adaptive")]      # (window as a share of L, method)


@functools.lru_cache(maxsize=None)
def _frames(m, length, b=2):
    """frames[b][m][length]: a common noise sequence with a delay per microphone, an echo of it and independent noise."""
    rng = np.random.default_rng([m, length])
    out = np.zeros((b, m, length))
    for f in range(b):
        common = rng.standard_normal(length + 64)
        for mic in range(m):
            d, e = rng.integers(0, min(24, length), 2)
            out[f, mic] = common[d:d + length] + 0.6 * np.roll(common[:length], int(e)) + 0.5 * rng.standard_normal(length)
    return out


@functools.lru_cache(maxsize=None)
def _rows(m, length):
    """The oracle's correlation rows of _frames(m, length): [b][P][2 length - 1]."""
    x = _frames(m, length)
    return np.stack([[O.phat_correlation(f[i], f[j]) for i, j in pair_list(m)] for f in x])


def _med(share, length):
    return None if share is None else share * length / FS


@functools.lru_cache(maxsize=None)
def _oracle(m, length, share, method, k=K):
    """-> (cand_k[b][P][k], cand_h, branch[b][P], n_sel, keep[b][P]: the pairs the parity rule compares)."""
    rows = _rows(m, length)
    b, p, _ = rows.shape
    cand_k = np.full((b, p, k), -1, dtype=np.int32)
    cand_h = np.zeros((b, p, k))
    branch = np.zeros((b, p), dtype=np.int32)
    keep = np.ones((b, p), dtype=bool)
    for f in range(b):
        for r in range(p):
            more, _ = O.select_peaks(rows[f, r], length, FS, k + 1, method, 1.0, _med(share, length))
            h = np.sort(rows[f, r][np.asarray(more, dtype=np.int64)])
            keep[f, r] = h.size < 2 or np.min(np.diff(h)) > MARGIN
            want, br = O.select_peaks(rows[f, r], length, FS, k, method, 1.0, _med(share, length))
            want = np.asarray(want, dtype=np.int64)
            cand_k[f, r, :want.size] = want
            cand_h[f, r, :want.size] = rows[f, r][want]
            branch[f, r] = br
    return cand_k, cand_h, branch, np.count_nonzero(cand_k >= 0, axis=2).astype(np.int32), keep


@pytest.fixture
def small_groups(engine):
    """Launch groups of two transforms (four pairs): ten pairs are three groups, the last one a single transform."""
    engine.set_chunk(2)
    yield engine
    engine.set_chunk(0)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("m", [3, 5])
def test_candidates_equal_the_oracles_selection(small_groups, m, length):
    engine = small_groups
    x = _frames(m, length)
    seen = 0
    for share, method in SETTINGS:
        want_k, want_h, want_br, want_n, keep = _oracle(m, length, share, method)
        assert np.count_nonzero(~keep) <= keep.size // 10, (m, length, share, method, "the parity rule drops more than a tenth of the pairs")
        table, cand_k, cand_h = engine.gcc_phat_all_pairs_peaks(x, FS, K, method, 1.0, _med(share, length))
        one = engine.gcc_phat_all_pairs(x, FS, 1, method, 1.0, _med(share, length))
        assert np.array_equal(cand_k[keep], want_k[keep]), (m, length, share, method)
        assert np.allclose(cand_h[keep], want_h[keep], **HEIGHT)
        assert np.array_equal(table["n_sel"][keep], want_n[keep]) and np.array_equal(table["branch"][keep], want_br[keep])
        for name in ("k_sel", "branch", "k_argmax"):                                          # the records are candidate 0's: the one-peak call's
            assert np.array_equal(table[name][keep], one[name][keep]), name
        assert np.array_equal(table["k_sel"], cand_k[..., 0]) and np.array_equal(table["sel_height"], cand_h[..., 0])
        absent = cand_k < 0
        assert np.all(cand_k[absent] == -1) and np.all(cand_h[absent] == 0.0) and not np.any(np.signbit(cand_h[absent]))
        assert np.array_equal(np.count_nonzero(~absent, axis=2), table["n_sel"])
        seen = max(seen, int(table["n_sel"].max()))
    assert seen == K or length < 64                                                           # the inputs have several peaks to select


def test_route_lengths_take_their_routes():
    """The kernels that ran say which route a several-peaks call of each of ROUTE_LENGTHS took.  On an engine of its own: profiling
    leaves kernel names behind, and other tests read the names of the shared engine."""
    from pyaudiolocalization_amd import Engine
    eng = Engine(0)
    try:
        for route, length in ROUTE_LENGTHS.items():
            eng.profile_begin()
            eng.gcc_phat_all_pairs_peaks(_frames(3, length), FS, K)
            eng.profile_end()
            ran = sorted(name for name, (_, launches) in eng.profile_entries().items() if launches > 0)
            print(f"[peaks] {route}, L = {length}: {ran}")
            fused = any(name.startswith("k_pfa_cols_stats") for name in ran)
            three = "k_peak_stream" in ran and "k_peak_pivots" in ran
            split = any(name.startswith("k_pfa") for name in ran)
            assert (fused, three, split) == {"kFused": (True, False, True), "kPfa": (False, True, True), "kFourStep": (False, True, False)}[route], (route, ran)
            assert "k_peak_finish" in ran
    finally:
        eng.close()


def test_other_peak_counts(small_groups):
    engine, m, length = small_groups, 5, 257
    x = _frames(m, length)
    for k in (1, 2, 8):
        want_k, want_h, _, want_n, keep = _oracle(m, length, None, "median", k)
        assert np.count_nonzero(~keep) <= keep.size // 10
        table, cand_k, cand_h = engine.gcc_phat_all_pairs_peaks(x, FS, k)
        assert cand_k.shape == (2, 10, k)
        assert np.array_equal(cand_k[keep], want_k[keep]) and np.allclose(cand_h[keep], want_h[keep], **HEIGHT)
        assert np.array_equal(table["n_sel"][keep], want_n[keep])
    one = engine.gcc_phat_all_pairs(x, FS)
    assert np.array_equal(engine.gcc_phat_all_pairs_peaks(x, FS, 1)[0]["k_sel"][keep], one["k_sel"][keep])


def test_argmax_fallbacks_give_one_candidate(small_groups):
    engine, m, length = small_groups, 5, 257
    x = _frames(m, length).copy()
    x[:, 2] = 0.0                                                                              # a silent microphone: its rows are all zero
    for med, pairs_hit in ((None, [p for p, (i, j) in enumerate(pair_list(m)) if 2 in (i, j)]), (0.0, list(range(10)))):
        table, cand_k, cand_h = engine.gcc_phat_all_pairs_peaks(x, FS, K, "median", 1.0, med)
        hit = table[:, pairs_hit]
        assert np.all(hit["branch"] & (_ffi.BR_ARGMAX_NO_PEAKS | _ffi.BR_ARGMAX_WINDOW)), (med, hit["branch"])
        assert np.all(hit["n_sel"] == 1)
        assert np.array_equal(cand_k[:, pairs_hit, 0], hit["k_sel"]) and np.all(cand_k[:, pairs_hit, 1:] == -1)
        rest = cand_h[:, pairs_hit, 1:]
        assert np.all(rest == 0.0) and not np.any(np.signbit(rest))
        for f, p in itertools.product(range(2), pairs_hit):
            i, j = pair_list(m)[p]
            want, br = O.select_peaks(O.phat_correlation(x[f, i], x[f, j]), length, FS, K, "median", 1.0, med)
            assert br == table["branch"][f, p] and len(want) == 1


def _dev_call(engine, x, prm, pairs=None):
    """The _dev forms around device buffers: all pairs of x[b][m][L], or the explicit pair list over the rows x[r][L]."""
    k = int(prm.num_peaks)
    shape = (pairs.shape[0],) if pairs is not None else (x.shape[0], x.shape[1] * (x.shape[1] - 1) // 2)
    table, cand_k, cand_h = np.zeros(shape, dtype=_ffi.RECORD), np.zeros(shape + (k,), dtype=np.int32), np.zeros(shape + (k,))
    bufs = [engine.alloc(a.nbytes) for a in (x, table, cand_k, cand_h)] + ([engine.alloc(pairs.nbytes)] if pairs is not None else [])
    try:
        engine.upload(bufs[0], x)
        if pairs is not None:
            engine.upload(bufs[4], pairs)
            engine.gcc_phat_pairs_peaks_dev(bufs[0], x.shape[0], x.shape[1], bufs[4], pairs.shape[0], prm, bufs[1], bufs[2], bufs[3])
        else:
            engine.gcc_phat_all_pairs_peaks_dev(bufs[0], x.shape[0], x.shape[1], x.shape[2], prm, bufs[1], bufs[2], bufs[3])
        engine.synchronize()
        for a, d in zip((table, cand_k, cand_h), bufs[1:4]):
            engine.download(a, d)
    finally:
        for d in bufs:
            engine.free(d)
    return table, cand_k, cand_h


@pytest.mark.parametrize("length", [257, ROUTE_LENGTHS["kFourStep"], ROUTE_LENGTHS["kPfa"]])
def test_dev_form_and_pair_list_equal_the_host_form(small_groups, length):
    engine, m = small_groups, 5
    x = _frames(m, length)
    for share, method in SETTINGS[1:3]:
        host = engine.gcc_phat_all_pairs_peaks(x, FS, K, method, 1.0, _med(share, length))
        prm = make_params(FS, K, method, 1.0, _med(share, length))
        dev = _dev_call(engine, x, prm)
        listed = _dev_call(engine, np.ascontiguousarray(x[1]), prm, pairs=pair_list(m))
        for name, h, d, l in zip(("table", "cand_k", "cand_h"), host, dev, listed):
            assert h.tobytes() == d.tobytes(), (name, "_dev")
            assert h[1].tobytes() == l.tobytes(), (name, "pair list")


def test_errors(engine):
    x = _frames(3, 64)
    for k in (0, 9):
        with pytest.raises(ValueError):
            engine.gcc_phat_all_pairs_peaks(x, FS, k)
        prm = make_params(FS, k)
        for call in (lambda: engine.gcc_phat_all_pairs_peaks_dev(0, 2, 3, 64, prm, 0, 0), lambda: engine.gcc_phat_pairs_peaks_dev(0, 3, 64, 0, 3, prm, 0, 0)):
            with pytest.raises(ValueError):
                call()
        out = np.zeros(64, dtype=np.int64)
        for symbol, args in (("pal_gcc_phat_all_pairs_peaks", (x.ctypes.data, 2, 3, 64)), ("pal_gcc_phat_all_pairs_peaks_dev", (x.ctypes.data, 2, 3, 64)),
                             ("pal_gcc_phat_pairs_peaks_dev", (x.ctypes.data, 3, 64, out.ctypes.data, 3))):
            rc = getattr(engine._lib, symbol)(engine._h, *args, C_.byref(prm), out.ctypes.data, out.ctypes.data, None)
            assert rc == _ffi.ERR_INVALID, (symbol, k)                                        # refused before any buffer is touched
    with pytest.raises(ValueError):
        engine.gcc_phat_all_pairs(x, FS, num_peaks=2)                                         # the one-peak call is as it was
    table, cand_k, _ = engine.gcc_phat_all_pairs_peaks(x[0], FS, K)                           # one frame: [P] and [P][K]
    assert table.shape == (3,) and cand_k.shape == (3, K)


def test_chain_simulate_peaks_consensus_solve(engine):
    """A two-plane scene, 8 microphones, 3000 samples: simulate -> four peaks per pair in one batched call -> centred indices -> consensus
    -> solve.  The direct path is the strongest (gain 0.49 against 0.07 for the reflections), so the first peaks are the true lags, which
    close every triangle within a sample once centred; what the chain buys in metres is printed, not asserted."""
    fs, nbase, m = 48000.0, 3000, 8
    pos = np.random.default_rng(55).uniform(-0.4, 0.4, (m, 3))
    delays, gains, longest, _ = O.multipath_paths(T.SRC, pos, cases.C_SOUND, 1000, cases.DEFAULT_PLANES[:2], cases.LOW_LOSS, 1, 0.01)
    base = np.random.default_rng(2000).standard_normal(nbase)
    frames = engine.simulate_multipath(base[None], fs, int((nbase / fs + longest) * fs), delays[None], gains[None], nbase)[0]
    table, cand_k, cand_h = engine.gcc_phat_all_pairs_peaks(frames, fs, K)
    assert np.all(table["n_sel"] >= 1) and np.array_equal(table["k_sel"], cand_k[:, 0])
    raw = engine.tdoa_consensus(cand_k, nbase, m, 1, 2, outputs=("summary",))[2][0]
    assert raw["closed_before"] == 0                                                          # under the reference's index mapping three first lags sum to about +-L
    centred = table.copy()
    centred["k_sel"] = CN.centred(table["k_sel"], nbase)
    sel, table_out, summary = engine.tdoa_consensus(CN.centred(cand_k, nbase), nbase, m, 1, 2, tables=centred, cand_h=cand_h)
    assert table_out.tobytes() == CN.apply(centred[None], CN.centred(cand_k, nbase)[None], cand_h[None], sel).tobytes()
    assert summary[0]["closed_after"] >= summary[0]["closed_before"] == m * (m - 1) * (m - 2) // 6
    rec = engine.solve_positions(table_out, nbase, pos, fs, cases.C_SOUND, buffer=T.BUFFER, grid=T.GRID)[0]
    print(f"[peaks] chain: {summary[0]['moved']} of {table.shape[0]} pairs moved, closed triangles {summary[0]['closed_before']} -> "
          f"{summary[0]['closed_after']}, {np.linalg.norm(rec['position'] - T.SRC):.4f} m from the source")
    assert np.all(np.isfinite(rec["position"]))
