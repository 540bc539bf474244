"""The Rader-row family on the device: every frame length L with 2 L - 1 = N1 x 991 runs k_pfa_fwd_cols,
k_pfa_fwd_rows_rader<11,9,10> and k_pfa_rows_rader<11,9,10> with a column pass behind them, and the code that depends on N1
(the forward column kernel's prefetch clamp, zero table rows and chunk guard, the row kernels' index arithmetic mod N1, the
host tables, the three column passes) is run here at the smallest N1 of every class (tests/rader_family.py), not only at
N1 = 1 and 89.  tests/test_host_rader_family.py pins the conditions on the inputs: the peak margins that make the exact index
comparisons meaningful, and that the amplitude-sensitive rows do move with the amplitude of a spectrum.

The engine under test is the session engine with no switch set.  PAL_PFA_FWD=0 (forward four-step, inverse Rader rows) and
PAL_RADER=0 (no Rader kernel on either side) are set only while a comparison engine is created: which of the two still
agrees with the oracle says which side a failure is on.  Every bound is one the suite already applies to the same operation:
1e-12 x max|want| and equal argmax against the oracle (test_prime_factor_route_matches_four_step_and_numpy), 1e-13 and equal
integer fields between routes (test_forward_spectra_through_the_prime_factor_cut), cmax at rtol 1e-11 and snr at rtol 1e-9
(test_prime_factor_route_odd_pair_counts_and_tables), 5e-14 on unequal lengths (the 600 + 392 case), equal bytes between the
two first-stage bodies (test_shared_and_four_row_bodies_are_bit_identical).  The worst row errors are printed per case;
profiles/rader_family_errors.txt keeps those of one run.
"""
import numpy as np
import pytest

from oracle import pal_oracle as O

import rader_family as RF
import row_scale as RS

pytestmark = pytest.mark.gpu

INT_FIELDS = ("k_sel", "branch", "k_argmax")
MED = 0.01
SHAPE_IDS = ["N1=%d-%s" % c for c in RF.SHAPE_CASES]
FWD_KERNELS = ("k_pfa_fwd_cols", "k_pfa_fwd_rows_rader<11,9,10>")
ROWS_KERNEL = "k_pfa_rows_rader<11,9,10>"
COLUMN_KERNELS = ("k_pfa_cols_stats", "k_pfa_cols_fin", "k_pfa_cols_lean", "k_pfa_cols")


def _second_engine(engine, monkeypatch, switch):
    """an engine created with `switch`=0; the variable is gone again before anything else runs"""
    from pyaudiolocalization_amd import Engine
    monkeypatch.setenv(switch, "0")
    try:
        return Engine(engine.device)
    finally:
        monkeypatch.delenv(switch)


def _profiled(eng, call):
    eng.profile_begin()
    try:
        out = call()
    finally:
        eng.profile_end()
    return out, {k: v for k, v in eng.profile_entries().items() if v[1] > 0}   # (names of earlier calls stay listed with no launches)


def _rows_against_oracle(corr, n1, shape, e=0):
    """every row within 1e-12 x max|want| of the oracle's, equal argmax; exact zeros for the silent microphone's pairs.
    Returns the worst |got - want| / max|want|."""
    b, m = RF.SHAPES[shape]
    worst = 0.0
    for f in range(b):
        for p, (i, j) in enumerate(RS.pairs_of(m)):
            want = RF.oracle_corr(n1, shape, f, i, j, e)
            if RF.silent_pair(shape, f, i, j):
                assert not want.any() and not corr[f, p].any(), (n1, shape, f, i, j)
                continue
            scale = float(np.max(np.abs(want)))
            err = float(np.max(np.abs(corr[f, p] - want))) / scale
            worst = max(worst, err)
            assert err <= 1e-12, (n1, shape, f, i, j, e, err)
            assert int(np.argmax(corr[f, p])) == int(np.argmax(want)), (n1, shape, f, i, j, e)
    return worst


# ================================================================================================ 1. plan and launches
@pytest.mark.parametrize("n1", RF.N1S)
def test_plan_and_launches(engine, n1):
    """The plan is N1 x 991 with the 990-point Rader tile, and a call that wants records only launches the packed forward
    transform, the Rader rows and the column pass of its class: the fused pass (k_pfa_cols_stats) for one chunk, the finishing
    pass (k_pfa_cols_fin) for two to four, the plain column kernel and the three statistics launches for five and six.
    Behind the finishing pass the profile may hold k_pfa_cols_stats as well: a row it hands on (pfa_cols_fin.h) is resolved by
    the stored-row path at the end of the call."""
    length = RF.length_of(n1)
    info = engine.plan_info(length)
    assert (info["n1"], info["n2"], info["tile_len"]) == (n1, RF.N2, RF.N2 - 1), info
    table, ent = _profiled(engine, lambda: engine.gcc_phat_all_pairs(RF.frames(n1, "narrow"), RF.FS, max_expected_delay=MED))
    for name in FWD_KERNELS + (ROWS_KERNEL,):
        assert name in ent and ent[name][1] >= 1, (name, sorted(ent))
    kernel = RF.column_kernel(n1)
    allowed = {kernel, "k_pfa_cols_stats"} if kernel == "k_pfa_cols_fin" else {kernel}
    assert kernel in ent and {k for k in COLUMN_KERNELS if k in ent} <= allowed, sorted(ent)
    if kernel == "k_pfa_cols":
        for name in ("k_peak_pivots", "k_peak_stream", "k_peak_finish"):
            assert name in ent, (name, sorted(ent))
    else:
        assert "k_peak_pivots" not in ent and "k_peak_stream" not in ent, sorted(ent)
    want = RF.oracle_table(n1, "narrow", 0, MED, "median")
    for key in INT_FIELDS:
        assert np.array_equal(table[0][key], want[key]), (n1, key)


# ================================================================================================ 2. rows
@pytest.mark.parametrize("n1,shape", RF.SHAPE_CASES, ids=SHAPE_IDS)
def test_rows_match_the_oracle_and_both_independent_routes(engine, n1, shape, monkeypatch):
    """Stored rows against the oracle, and against an engine whose forward spectra take the four-step route (PAL_PFA_FWD=0) and
    one without a Rader kernel on either side (PAL_RADER=0)."""
    length, fr = RF.length_of(n1), RF.frames(n1, shape)
    call = lambda eng: eng.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=MED, want_corr=True)
    (t1, c1), ent = _profiled(engine, lambda: call(engine))
    for name in FWD_KERNELS + (ROWS_KERNEL,):
        assert name in ent, (name, sorted(ent))
    worst = _rows_against_oracle(c1, n1, shape)
    others = {}
    for switch in ("PAL_PFA_FWD", "PAL_RADER"):
        plain = _second_engine(engine, monkeypatch, switch)
        try:
            assert plain.plan_info(length)["tile_len"] == (RF.N2 - 1 if switch == "PAL_PFA_FWD" else 2048)
            (t0, c0), ent0 = _profiled(plain, lambda: call(plain))
        finally:
            plain.close()
        for name in FWD_KERNELS:
            assert name not in ent0, (switch, name, sorted(ent0))
        assert (ROWS_KERNEL in ent0) == (switch == "PAL_PFA_FWD"), (switch, sorted(ent0))
        _rows_against_oracle(c0, n1, shape)
        others[switch] = float(np.max(np.abs(c1 - c0)))
        assert others[switch] <= 1e-13, (n1, shape, switch, others[switch])
        for key in INT_FIELDS + ("n_sel",):
            assert np.array_equal(t1[key], t0[key]), (n1, shape, switch, key)
    print("rader family N1 = %d %s: worst row error %.3g of max|want| against the oracle; %.3g / %.3g absolute against "
          "PAL_PFA_FWD=0 / PAL_RADER=0" % (n1, shape, worst, others["PAL_PFA_FWD"], others["PAL_RADER"]))


# ================================================================================================ 3. records without stored rows
@pytest.mark.parametrize("n1,shape", RF.SHAPE_CASES, ids=SHAPE_IDS)
def test_records_without_stored_rows(engine, n1, shape, monkeypatch, capfd):
    """The call the finishing pass serves: both windows, both methods, every record against the oracle's table.  The finishing
    pass may hand a row to the stored-row path at the end of the call (pfa_cols_fin.h: the exact zero rows of the silent
    microphone are ties, a window peak may sit at the window's edge); its report (PAL_DEBUG_FALLBACK=1) must leave rows of every
    call to the pass itself - on one run it kept every row but those - and the other two column passes hand on nothing."""
    from test_gpu_peak_positions import _flag_report
    monkeypatch.setenv("PAL_DEBUG_FALLBACK", "1")                   # (read at every report, not at creation)
    fr = RF.frames(n1, shape)
    handed = []
    for med in RF.MEDS:
        for method in RF.METHODS:
            engine.synchronize()                                    # (reports and clears what earlier calls left in the status words)
            capfd.readouterr()
            table, ent = _profiled(engine, lambda: engine.gcc_phat_all_pairs(fr, RF.FS, 1, method, 1.0, med))
            rep = _flag_report(capfd.readouterr().err)
            assert RF.column_kernel(n1) in ent, sorted(ent)
            handed.append("%s %s: %s" % (med, method, ", ".join("%s %d" % kv for kv in rep.items() if kv[1]) or "none"))
            if RF.column_kernel(n1) == "k_pfa_cols_fin":
                assert rep["flagged"] < table.size, rep
            else:
                assert rep["flagged"] == 0, rep
            for f in range(fr.shape[0]):
                want = RF.oracle_table(n1, shape, f, med, method)
                tag = (n1, shape, f, med, method)
                for key in INT_FIELDS:
                    assert np.array_equal(table[f][key], want[key]), (tag, key, table[f][key].tolist(), want[key].tolist())
                assert np.allclose(table[f]["cmax"], want["cmax"], rtol=1e-11, atol=0), (tag, table[f]["cmax"] - want["cmax"])
                assert np.allclose(table[f]["snr"], want["snr"], rtol=1e-9, atol=0), (tag, table[f]["snr"] / want["snr"] - 1)
    if RF.column_kernel(n1) == "k_pfa_cols_fin":
        print("rader family N1 = %d %s: rows handed on by the finishing pass: %s" % (n1, shape, "; ".join(handed)))


# ================================================================================================ 4. amplitude-sensitive rows
@pytest.mark.parametrize("n1", RF.AMPLITUDE)
def test_amplitude_sensitive_rows(engine, n1):
    """Every microphone at 2^e with 4^e L ~ 1e-10: the whitening R / (|R| + 1e-10) no longer divides the amplitude of the
    spectra out (the oracle's row moves by 0.4 ... 0.7 of its maximum, host test), so an amplitude error of the packed forward
    transform - its column sums, its power-of-two rescale - shows in the row."""
    e = RF.amplitude_exponent(n1)
    fr = RF.frames(n1, "narrow") * 2.0 ** e
    (table, corr), ent = _profiled(engine, lambda: engine.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=MED, want_corr=True))
    for name in FWD_KERNELS + (ROWS_KERNEL,):
        assert name in ent, (name, sorted(ent))
    worst = _rows_against_oracle(corr, n1, "narrow", e)
    print("rader family N1 = %d narrow at 2^%d: worst row error %.3g of max|want| against the oracle" % (n1, e, worst))


# ================================================================================================ 5. unequal lengths
UNEQUAL_CASES = [(n1,) + c for n1 in RF.UNEQUAL for c in RF.unequal_cases(n1)]


@pytest.mark.parametrize("n1,tag,len1,len2,launches", UNEQUAL_CASES, ids=["N1=%d-%s" % c[:2] for c in UNEQUAL_CASES])
def test_unequal_lengths_through_phat_correlation(engine, n1, tag, len1, len2, launches):
    """A signal takes the packed forward transform while (len - 1) // 991 <= h and the four-step storer beyond: both spectra
    through the cut with the first at the rule's upper edge (two launches of k_pfa_fwd_cols), one spectrum from each producer
    in the same permuted layout (one launch), a one-sample signal, and a second signal shorter than one column block."""
    a, b = RF.unequal_signals(n1, tag, len1, len2)
    assert engine.plan_info((len1 + len2) // 2)["n1"] == n1 and len1 + len2 - 1 == n1 * RF.N2
    got, ent = _profiled(engine, lambda: engine.phat_correlation(a, b))
    want = O.phat_correlation(a, b)
    err = float(np.max(np.abs(got - want)))
    print("rader family N1 = %d %s (%d + %d samples): %.3g absolute, %s launches of k_pfa_fwd_cols"
          % (n1, tag, len1, len2, err, ent.get("k_pfa_fwd_cols", (0.0, 0))[1]))
    assert ROWS_KERNEL in ent, sorted(ent)
    assert got.shape == want.shape and err <= 5e-14, (n1, tag, err)
    if launches is not None:
        assert ent.get("k_pfa_fwd_cols", (0.0, 0))[1] == launches, (n1, tag, sorted(ent))
        assert ent.get("k_pfa_fwd_rows_rader<11,9,10>", (0.0, 0))[1] == launches, (n1, tag, sorted(ent))


# ================================================================================================ 6. both first-stage bodies
@pytest.mark.parametrize("n1", RF.BODIES)
def test_shared_and_four_row_bodies_are_bit_identical(engine, n1, monkeypatch):
    """B = 2, M = 4: six pairs per frame pack as (01,02) - shared first microphone - then (03,12) and (13,23), which keep the
    four-row body; frame 1's transforms point at rows offset by M.  With and without a silent shared microphone:
    PAL_ROWS_SHARED=0 never takes the shared body, and every record and every stored sample is bit-identical."""
    five = RF.five_microphones(n1)
    two = np.stack([five[:4], five[1:]])
    silent = two.copy()
    silent[0, 0] = 0.0
    plain = _second_engine(engine, monkeypatch, "PAL_ROWS_SHARED")
    try:
        for fr in (two, silent):
            for med in (MED, None):
                a = engine.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=med)
                b = plain.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=med)
                assert a.tobytes() == b.tobytes(), (n1, med)
            a, ca = engine.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=MED, want_corr=True)
            b, cb = plain.gcc_phat_all_pairs(fr, RF.FS, max_expected_delay=MED, want_corr=True)
            assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes(), n1
        assert not ca[0, :3].any() and np.all(np.max(np.abs(ca[0, 3:]), axis=1) > 0.01) and np.all(np.max(np.abs(ca[1]), axis=1) > 0.01)
    finally:
        plain.close()
