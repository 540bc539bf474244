#!/usr/bin/env python3
"""Loop-closure consensus over K = 4 candidates per pair on ONE GPU (csrc/consensus.hip): 128 frames x 64 microphones and
16 frames x 256 microphones, candidate tables resident in HBM; per frame a source of its own, its lag in slot 0 of half of the pairs and in a
random other slot of the rest, every other candidate a lag within +-2400 samples.

    python tools/bench_consensus.py [repeats=5]

Writes one JSON to profiles/consensus_bench.json and prints it: per workload the device call (Engine.tdoa_consensus_dev with all three
outputs in HBM, tol 1, two rounds, then synchronize; best of `repeats` after a warm-up call), the kernel times of pal_profile, the NumPy
specification's time per frame on the first frames of the same tables (consensus.tdoa_consensus, checked equal to the device's outputs) and
Engine.tdoa_closure_dev on the same tables.  No speed is promised; those two are the yardsticks.  Then the call that makes the
candidates: pal_gcc_phat_all_pairs_peaks_dev with K = 4 against the one-peak pal_gcc_phat_all_pairs_dev on C5-sized frames (16 frames x
64 microphones x 12000 samples at 48 kHz, lag window 0.05 s) - the one-peak call takes the finishing pass that a several-peaks call cannot."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import RECORD, Engine, closure, consensus, make_params  # noqa: E402
from pyaudiolocalization_amd.engine import pair_list  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fs, L, c, K, TOL, ROUNDS = 48000.0, 12000, cases.C_SOUND, 4, 1, 2
eng = Engine(0)


def best_of(call):
    call()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    return best


def workload(frames, mics_n, spec_frames):
    rng = np.random.default_rng([11, mics_n])
    mics = cases.fibonacci_sphere(mics_n, 0.5)
    pl = pair_list(mics_n)
    p = len(pl)
    sources = rng.uniform(-3, 3, (frames, 3)) + np.array([0, 0, 1.5])
    cand = rng.integers(-2400, 2401, (frames, p, K))
    slot = np.where(rng.random((frames, p)) < 0.5, rng.integers(1, K, (frames, p)), 0)
    for f in range(frames):
        d = np.linalg.norm(mics - sources[f], axis=1)
        cand[f, np.arange(p), slot[f]] = np.rint((d[pl[:, 1]] - d[pl[:, 0]]) / c * fs).astype(np.int64)
    cand_k = np.ascontiguousarray(cand + (L - 1), dtype=np.int32)
    cand_h = np.ascontiguousarray(rng.random((frames, p, K)))
    tables = np.zeros((frames, p), dtype=RECORD)
    tables["k_sel"] = cand_k[..., 0]
    tables["snr"] = 1.0
    out = [np.zeros((frames, p), dtype=np.int32), np.zeros((frames, p), dtype=RECORD), np.zeros(frames, dtype=consensus.SUMMARY)]
    d_in = [eng.alloc(a.nbytes) for a in (cand_k, tables, cand_h)]
    d_out = [eng.alloc(a.nbytes) for a in out]
    for a, d in zip((cand_k, tables, cand_h), d_in):
        eng.upload(d, a)

    def call():
        eng.tdoa_consensus_dev(d_in[0], frames, mics_n, K, L, TOL, ROUNDS, d_tables=d_in[1], d_cand_h=d_in[2], d_sel=d_out[0],
                               d_table_out=d_out[1], d_summary=d_out[2])
        eng.synchronize()

    best = best_of(call)
    eng.profile_begin()
    call()
    eng.profile_end()
    kernels = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in eng.profile_entries().items() if k.startswith(("k_consensus", "k_closure_votes"))}   # the summary's two vote passes are closure.hip's kernel
    for a, d in zip(out, d_out):
        eng.download(a, d)
    t0 = time.perf_counter()
    want_sel, want_sum = consensus.tdoa_consensus(cand_k[:spec_frames], L, mics_n, TOL, ROUNDS)
    spec_s = (time.perf_counter() - t0) / spec_frames
    want_tab = consensus.apply(tables[:spec_frames], cand_k[:spec_frames], cand_h[:spec_frames], want_sel)
    equal = all(a[:spec_frames].tobytes() == w.tobytes() for a, w in zip(out, (want_sel, want_tab, want_sum)))
    right = np.count_nonzero(out[0] == slot) / slot.size

    d_votes = eng.alloc(frames * p * 4)
    d_sum = eng.alloc(frames * closure.SUMMARY.itemsize)
    closure_s = best_of(lambda: (eng.tdoa_closure_dev(d_in[1], frames, mics_n, L, TOL, 1, "soft", d_votes=d_votes, d_summary=d_sum), eng.synchronize()))
    res = {"frames": frames, "mics": mics_n, "pairs": p, "candidates": K, "tol": TOL, "rounds": ROUNDS, "repeats": repeats,
           "stage0_tests_per_frame": p * (mics_n - 2) * K ** 3, "device_seconds_per_call": round(best, 6), "frames_per_s": round(frames / best, 1),
           "kernels": kernels, "numpy_specification_seconds_per_frame": round(spec_s, 4), "specification_frames": spec_frames,
           "device_equals_specification": bool(equal), "tdoa_closure_dev_seconds_per_call": round(closure_s, 6),
           "pairs_on_the_true_slot": round(right, 6), "first_picks_on_the_true_slot": round(float(np.mean(slot == 0)), 6),
           "closed_before_mean": float(np.mean(out[2]["closed_before"])), "closed_after_mean": float(np.mean(out[2]["closed_after"])),
           "changed_last_mean": float(np.mean(out[2]["changed_last"]))}
    for d in d_in + d_out + [d_votes, d_sum]:
        eng.free(d)
    return res


def peaks_timing(frames=16, mics_n=64, length=12000, fs_hz=48000.0, med=0.05):
    rng = np.random.default_rng(5)
    common = rng.standard_normal((frames, length + 256))
    x = np.stack([[common[f, d:d + length] + 0.5 * rng.standard_normal(length) for d in rng.integers(0, 200, mics_n)] for f in range(frames)])
    p = mics_n * (mics_n - 1) // 2
    bufs = [eng.alloc(n) for n in (x.nbytes, frames * p * RECORD.itemsize, frames * p * K * 4, frames * p * K * 8)]
    eng.upload(bufs[0], x)
    one, many = make_params(fs_hz, 1, "median", 1.0, med), make_params(fs_hz, K, "median", 1.0, med)
    t_one = best_of(lambda: (eng.gcc_phat_all_pairs_dev(bufs[0], frames, mics_n, length, one, bufs[1]), eng.synchronize()))
    first = eng.download(np.zeros((frames, p), dtype=RECORD), bufs[1]).copy()
    t_many = best_of(lambda: (eng.gcc_phat_all_pairs_peaks_dev(bufs[0], frames, mics_n, length, many, bufs[1], bufs[2], bufs[3]), eng.synchronize()))
    table = eng.download(np.zeros((frames, p), dtype=RECORD), bufs[1])
    cand_k = eng.download(np.zeros((frames, p, K), dtype=np.int32), bufs[2])
    for d in bufs:
        eng.free(d)
    return {"frames": frames, "mics": mics_n, "length": length, "pairs_per_call": frames * p, "candidates": K, "repeats": repeats,
            "one_peak_seconds_per_call": round(t_one, 6), "one_peak_pairs_per_s": round(frames * p / t_one, 1),
            "peaks_seconds_per_call": round(t_many, 6), "peaks_pairs_per_s": round(frames * p / t_many, 1),
            "first_candidate_equals_one_peak_table": bool(np.array_equal(table["k_sel"], first["k_sel"]) and np.array_equal(cand_k[..., 0], first["k_sel"])),
            "mean_candidates_per_pair": float(np.mean(table["n_sel"]))}


result = {"workloads": [workload(128, 64, 8), workload(16, 256, 1)], "peaks_call": peaks_timing()}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "consensus_bench.json"), "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
eng.close()
