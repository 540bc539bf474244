"""Rows that share one packed complex transform must not see their partner's amplitude.

One row of every input is scaled by 2^e, e in {-40, -20, +20, +40}, and moved through every position of the packing
(tests/row_scale.py).  The reference transforms every row on its own, so its result for a row does not depend on any other
row and its error is relative to that row's own scale (tests/test_host_row_scale.py pins this, and the peak margins that
make the exact index comparisons meaningful).  Every bound is the one the suite already applies to the same operation at
unit scale: 1e-13 on PHAT rows, rtol 1e-10 / atol 1e-14 on cmax / cmin and rtol 1e-8 on snr (test_all_pairs_small_batches);
4e-15 on rows and rtol 1e-11 / atol 1e-15 on float fields for "another partner in the packed transform"; 1e-10 on
correlation values, 1e-12 on fractional_delay (both relative to the row's own scale: the reference is exactly covariant),
1e-11 on the normalised multipath rows; rtol 1e-10 on bootstrap peaks.
"""
import contextlib
import os

import numpy as np
import pytest

from oracle import pal_oracle as O

import row_scale as RS

pytestmark = pytest.mark.gpu

INT_FIELDS = ("k_sel", "branch", "k_argmax")
FLOAT_FIELDS = ("cmax", "cmin", "snr", "sel_height")


@pytest.fixture(scope="module")
def engine_fwd0(engine):
    """one frame per forward transform (PAL_PFA_FWD=0, read when the engine is created): the independent route"""
    from pyaudiolocalization_amd import Engine
    old = os.environ.get("PAL_PFA_FWD")
    os.environ["PAL_PFA_FWD"] = "0"
    try:
        eng = Engine(engine.device)
    finally:
        if old is None:
            del os.environ["PAL_PFA_FWD"]
        else:
            os.environ["PAL_PFA_FWD"] = old
    yield eng
    eng.close()


@contextlib.contextmanager
def _device(engine, *hosts):
    ptrs = []
    try:
        for h in hosts:
            arr = np.ascontiguousarray(h, dtype=np.float64)
            ptrs.append(engine.alloc(max(8, arr.nbytes)))
            engine.upload(ptrs[-1], arr)
        yield ptrs
    finally:
        for p in ptrs:
            engine.free(p)


# ================================================================================================ PHAT
_PLAIN = {}


def _plain(eng, tag, name, nframes, med, method):
    """the engine's own result on the unscaled frames"""
    key = (tag, name, nframes, med, method)
    if key not in _PLAIN:
        fs = RS.PHAT_SHAPES[name][3]
        _PLAIN[key] = eng.gcc_phat_all_pairs(RS.phat_frames(name)[:nframes], fs, 1, method, 1.0, med, want_corr=True)
    return _PLAIN[key]


def _check_records(table, want, tag):
    for key in INT_FIELDS:
        assert np.array_equal(table[key], want[key]), (tag, key, table[key].tolist(), want[key].tolist())
    assert np.allclose(table["cmax"], want["cmax"], rtol=1e-10, atol=1e-14), (tag, "cmax", table["cmax"] - want["cmax"])
    assert np.allclose(table["cmin"], want["cmin"], rtol=1e-10, atol=1e-14), (tag, "cmin", table["cmin"] - want["cmin"])
    assert np.allclose(table["snr"], want["snr"], rtol=1e-8), (tag, "snr", table["snr"] / want["snr"] - 1)


def _phat_case(eng, etag, name, pos):
    _, m, _, fs = RS.PHAT_SHAPES[name]
    ptag, nframes, mic = pos
    pairs = RS.pairs_of(m)
    touched = set(RS.pairs_with(m, mic))
    worst_row, worst_own = 0.0, 0.0
    for e in RS.EXPS:
        frames = RS.scaled_frames(name, nframes, mic, e)
        for med in RS.MEDS:
            for method in RS.METHODS:
                tag = (etag, name, ptag, e, med, method)
                table, corr = eng.gcc_phat_all_pairs(frames, fs, 1, method, 1.0, med, want_corr=True)
                table0, corr0 = _plain(eng, etag, name, nframes, med, method)
                for f in range(nframes):
                    _check_records(table[f], RS.oracle_table(name, f, {mic: e} if f == 0 else {}, med, method), tag + (f,))
                    for p, (i, j) in enumerate(pairs):
                        hit = f == 0 and p in touched
                        want = RS.oracle_corr(name, f, i, j, e if hit and i == mic else 0, e if hit and j == mic else 0)
                        err = float(np.max(np.abs(corr[f, p] - want)))
                        worst_row = max(worst_row, err)
                        assert err <= 1e-13, (tag, f, i, j, err)
                        if not hit:                                  # against the engine's own result on the unscaled input
                            own = float(np.max(np.abs(corr[f, p] - corr0[f, p])))
                            worst_own = max(worst_own, own)
                            assert own <= 4e-15, (tag, f, i, j, own)
                            for key in INT_FIELDS + ("n_sel",):
                                assert table[f][p][key] == table0[f][p][key], (tag, f, i, j, key)
                            for key in FLOAT_FIELDS:
                                assert np.isclose(table[f][p][key], table0[f][p][key], rtol=1e-11, atol=1e-15), (tag, f, i, j, key)
        # an explicit pair list: an untouched pair beside pairs of the scaled microphone (three pairs: a half-empty transform)
        others = [q for q in range(m) if q != mic]
        plist = [(others[0], others[1]), tuple(sorted((mic, others[0]))), tuple(sorted((others[2], mic)))]
        for med in RS.MEDS:
            for method in RS.METHODS:
                tag = (etag, name, ptag, e, med, method, "pairs")
                sub = eng.gcc_phat_pairs(frames[0], plist, fs, method, 1.0, med)
                sub0 = eng.gcc_phat_pairs(RS.phat_frames(name)[0], plist, fs, method, 1.0, med)
                for p, (i, j) in enumerate(plist):
                    want = RS.oracle_record(name, 0, i, j, e if i == mic else 0, e if j == mic else 0, med, method)
                    _check_records(sub[p:p + 1], {k: np.array([v]) for k, v in want.items()}, tag + (i, j))
                for key in INT_FIELDS + ("n_sel",):
                    assert sub[0][key] == sub0[0][key], (tag, key)
                for key in FLOAT_FIELDS:
                    assert np.isclose(sub[0][key], sub0[0][key], rtol=1e-11, atol=1e-15), (tag, key)
    print("%s %s %s: worst row error %.3g against the oracle, %.3g against the unscaled run (untouched pairs)"
          % (etag, name, ptag, worst_row, worst_own))


PHAT_CASES = [(name, pos) for name in RS.PHAT_SHAPES for pos in RS.phat_positions(name)]


@pytest.mark.parametrize("name,pos", PHAT_CASES, ids=["%s-%s" % (n, p[0]) for n, p in PHAT_CASES])
def test_phat_rows_do_not_see_a_scaled_partner(engine, name, pos):
    _phat_case(engine, "default", name, pos)


FWD0_CASES = [(n, p) for n, p in PHAT_CASES if n in ("rader496", "head44100")]


@pytest.mark.parametrize("name,pos", FWD0_CASES, ids=["%s-%s" % (n, p[0]) for n, p in FWD0_CASES])
def test_phat_rows_one_frame_per_forward_transform(engine_fwd0, name, pos):
    engine_fwd0.profile_begin()
    engine_fwd0.gcc_phat_all_pairs(RS.phat_frames(name)[:1], RS.PHAT_SHAPES[name][3])
    engine_fwd0.profile_end()
    assert "k_pfa_fwd_cols" not in engine_fwd0.profile_entries()
    _phat_case(engine_fwd0, "fwd0", name, pos)


@pytest.mark.parametrize("pos", RS.phat_positions("head44100"), ids=[p[0] for p in RS.phat_positions("head44100")])
def test_headline_route_records_without_stored_rows(engine, pos):
    """L = 44 100 without want_corr: the packed forward transform and the finishing column pass, records only"""
    name = "head44100"
    _, m, _, fs = RS.PHAT_SHAPES[name]
    for ptag, nframes, mic in (pos,):
        for e in RS.EXPS:
            frames = RS.scaled_frames(name, nframes, mic, e)
            for med in RS.MEDS:
                for method in RS.METHODS:
                    engine.profile_begin()
                    table = engine.gcc_phat_all_pairs(frames, fs, 1, method, 1.0, med)
                    engine.profile_end()
                    ent = engine.profile_entries()
                    assert ent["k_pfa_fwd_cols"][1] >= 1 and any(k.startswith("k_pfa_cols_fin") for k in ent), sorted(ent)
                    _check_records(table[0], RS.oracle_table(name, 0, {mic: e}, med, method), (ptag, e, med, method))


@pytest.mark.parametrize("name", RS.QUIET_SHAPES)
def test_quiet_pair_beside_a_loud_one_in_the_inverse(engine, name):
    """two microphones at 2^QUIET_EXP: their whitened pair is far smaller than the pair packed beside it in the PHAT inverse"""
    _, m, _, fs = RS.PHAT_SHAPES[name]
    e = RS.QUIET_EXP[name]
    frames = np.array(RS.phat_frames(name)[:1])
    for q in RS.QUIET_MICS:
        frames[0, q] *= 2.0 ** e
    p = RS.pairs_of(m).index(RS.QUIET_MICS)
    for med in RS.MEDS:
        for method in RS.METHODS:
            table = engine.gcc_phat_all_pairs(frames, fs, 1, method, 1.0, med)
            want = RS.oracle_record(name, 0, RS.QUIET_MICS[0], RS.QUIET_MICS[1], e, e, med, method)
            for key in INT_FIELDS:
                assert table[0][p][key] == want[key], (name, e, med, method, key, int(table[0][p][key]), want[key])


# ================================================================================================ xcorr / sync
def _check_xcorr(measured, exact, ref, tag):
    kpk, win, pk, refpk = measured
    worst = 0.0
    for q, seq in enumerate(exact):
        at = int(np.argmax(np.abs(seq)))
        peak = float(abs(seq[at]))
        tol = 1e-10 * peak                                           # relative to the row's own exact peak
        assert int(kpk[q]) == at, (tag, q, int(kpk[q]), at)
        worst = max(worst, abs(pk[q] - peak) / peak)
        assert abs(pk[q] - peak) <= tol, (tag, q, "pkabs", abs(pk[q] - peak) / peak)
        for j in range(5):
            p = at + j - 2
            if 0 <= p < seq.shape[0]:
                worst = max(worst, abs(win[q, j] - seq[p]) / peak)
                assert abs(win[q, j] - seq[p]) <= tol, (tag, q, j, abs(win[q, j] - seq[p]) / peak)
            else:
                assert np.isnan(win[q, j]), (tag, q, j)
    assert refpk == pk[ref], tag
    return worst


def _check_unscaled_rows(measured, plain, exact, skip, tag):
    """rows other than the scaled one: within the same bound of their results on the unscaled input"""
    for q, seq in enumerate(exact):
        if q == skip:
            continue
        tol = 1e-10 * float(np.max(np.abs(seq)))
        assert int(measured[0][q]) == int(plain[0][q]), (tag, q)
        assert abs(measured[2][q] - plain[2][q]) <= tol, (tag, q)
        ok = ~np.isnan(plain[1][q])
        assert np.array_equal(np.isnan(measured[1][q]), ~ok) and np.all(np.abs(measured[1][q][ok] - plain[1][q][ok]) <= tol), (tag, q)


@pytest.mark.parametrize("r", RS.XCORR_R)
def test_xcorr_vs_ref_rows_of_unequal_scale(engine, r):
    rows = RS.xcorr_rows(r)
    worst = 0.0
    for ref in RS.xcorr_refs(r):
        plain = engine.xcorr_vs_ref(rows, ref)
        exact0 = RS.xcorr_exact(rows, ref)
        _check_xcorr(plain, exact0, ref, (r, ref, "plain"))
        for at in RS.xcorr_positions(r, ref):
            for e in RS.EXPS:
                x = np.array(rows)
                x[at] *= 2.0 ** e
                got = engine.xcorr_vs_ref(x, ref)
                worst = max(worst, _check_xcorr(got, RS.xcorr_exact(x, ref), ref, (r, ref, at, e)))
                if at != ref:                                        # (a scaled reference scales every row's result)
                    _check_unscaled_rows(got, plain, exact0, at, (r, ref, at, e))
    print("xcorr R=%d: worst error relative to the row's peak %.3g" % (r, worst))


def test_sync_measure_dev_rows_of_unequal_scale(engine):
    frames = RS.sync_frames()
    with _device(engine, frames) as (d_rows,):
        ref0, kpk0, win0, pk0, refpk0 = engine.sync_measure_dev(d_rows, RS.SYNC_B, RS.SYNC_M, RS.XCORR_N)
    assert ref0.tolist() == list(RS.SYNC_LOUD)
    exact0 = [RS.xcorr_exact(frames[g], RS.SYNC_LOUD[g]) for g in range(RS.SYNC_B)]
    for g in range(RS.SYNC_B):
        _check_xcorr((kpk0[g], win0[g], pk0[g], refpk0[g]), exact0[g], RS.SYNC_LOUD[g], ("sync", "plain", g))
    for f, q in RS.SYNC_SCALED:
        for e in RS.EXPS:
            x = np.array(frames)
            x[f, q] *= 2.0 ** e
            refs = [RS.numpy_ref(fr) for fr in x]
            assert refs[f] == (q if e > 0 else RS.SYNC_LOUD[f])      # the scaled row is the reference row when it is louder
            with _device(engine, x) as (d_rows,):
                ref, kpk, win, pk, refpk = engine.sync_measure_dev(d_rows, RS.SYNC_B, RS.SYNC_M, RS.XCORR_N)
            assert ref.tolist() == refs
            for g in range(RS.SYNC_B):
                _check_xcorr((kpk[g], win[g], pk[g], refpk[g]), RS.xcorr_exact(x[g], refs[g]), refs[g], ("sync", f, q, e, g))
                # against the run on the unscaled frames: every other frame, and the scaled frame's other rows while its
                # reference row is the same one (e < 0; a louder scaled row becomes the reference and scales every result)
                if g != f or e < 0:
                    _check_unscaled_rows((kpk[g], win[g], pk[g]), (kpk0[g], win0[g], pk0[g]), exact0[g], q if g == f else -1,
                                         ("sync", f, q, e, g))


# ================================================================================================ fractional_delay
def test_fractional_delay_rows_of_unequal_scale(engine):
    from test_gpu_second_path import FD_DELAYS
    assert np.array_equal(FD_DELAYS, RS.FD_DELAYS)
    rows = RS.fd_rows()
    want = [O.fractional_delay(rows[q], RS.FD_DELAYS[q], RS.FD_FS) for q in range(RS.FD_R)]
    worst = 0.0
    for at in RS.FD_POSITIONS:
        for e in RS.EXPS:
            x = np.array(rows)
            x[at] *= 2.0 ** e
            got = engine.fractional_delay(x, RS.FD_DELAYS, RS.FD_FS)
            for q in range(RS.FD_R):
                k = 2.0 ** (e if q == at else 0)                     # (O.fractional_delay of the scaled row: exactly k x, host test)
                top = float(np.max(np.abs(x[q])))
                err = float(np.max(np.abs(got[q] - want[q] * k))) / top
                worst = max(worst, err)
                assert err <= 1e-12, (at, e, q, err)
    print("fractional_delay: worst error relative to max|row| %.3g" % worst)


# ================================================================================================ simulate_multipath
def test_simulate_multipath_bases_of_unequal_scale(engine):
    base, delays, gains = RS.sim_tables()
    rows, out_len = RS.SIM_B * RS.SIM_M, RS.SIM_TOTAL
    worst = 0.0
    for f in range(RS.SIM_B):
        for e in RS.SIM_EXPS:
            x = np.array(base)
            x[f] *= 2.0 ** e
            got = engine.simulate_multipath(x, RS.SIM_FS, RS.SIM_TOTAL, delays, gains)
            with _device(engine, x, delays, gains, np.zeros(rows * out_len)) as (d_base, d_delays, d_gains, d_out):
                engine.simulate_multipath_dev(d_base, RS.SIM_B, RS.SIM_NBASE, RS.SIM_FS, RS.SIM_TOTAL, d_delays, d_gains, RS.SIM_M,
                                              RS.SIM_K, 0, d_out)
                engine.synchronize()
                dev = engine.download(np.empty(rows * out_len), d_out).reshape(got.shape)
                kept = engine.download(np.empty(gains.size), d_gains)
            assert kept.tobytes() == gains.tobytes()                 # the caller's gain table is not rescaled in place
            for g in range(RS.SIM_B):
                want = RS.sim_want(g)                                # (the oracle normalises: the same bits for a scaled base, host test)
                for tag, arr in (("host", got), ("dev", dev)):
                    err = float(np.max(np.abs(arr[g] - want)))
                    worst = max(worst, err)
                    assert err <= 1e-11, (tag, f, e, g, err)
    print("simulate_multipath: worst error %.3g" % worst)


# ================================================================================================ bootstrap
BOOT_CASES = {"issue": (0, 8),      # the issue's case: rows[0] loud.  Its partner in the forward packing, rows[1], is used only
                                    # through its shuffles, which are transformed at unit scale in a call of their own, so this case
                                    # meets no packing of unequal rows (it passed before the rescale)
              "partner": (1, 7)}    # rows[1] loud: the quiet rows[0], whose unshuffled spectrum IS used, rides with it; and with an
                                    # odd count the last shuffle of the loud rows[1] shares a transform with the first of rows[3]


@pytest.mark.parametrize("case", sorted(BOOT_CASES))
def test_bootstrap_peaks_beside_a_loud_row(engine, case):
    from pyaudiolocalization_amd import bootstrap as B
    loud, count = BOOT_CASES[case]
    rows = np.array(RS.phat_frames("rader496")[0, :4])
    rows[loud] *= 2.0 ** 30
    pairs = np.array([[0, 1], [2, 3]], dtype=np.int32)
    mode, block, seed = "permutation", 50, 3
    got = engine.bootstrap_peaks(rows, pairs, count, mode, block, seed=seed)
    want = np.empty((2, count))
    for p, (i, j) in enumerate(pairs):                               # as test_gpu_bootstrap.py's _oracle_peaks
        for s in range(count):
            perm = B.shuffle_indices(rows.shape[1], i, j, s, mode, block, seed)
            want[p, s] = np.max(O.phat_correlation(rows[i], rows[j][perm]))
    print("bootstrap %s: worst relative error %.3g" % (case, float(np.max(np.abs(got / want - 1)))))
    assert np.allclose(got, want, rtol=1e-10, atol=0)
