#!/usr/bin/env python3
"""Loop-closure check of TDOA tables on ONE GPU (csrc/closure.hip): 128 frames x 64 microphones and 16 frames x 256
microphones, tables resident in HBM, a tenth of the pairs of every frame replaced by a lag within +-2400 samples.

    python tools/bench_closure.py [repeats=5]

Writes one JSON to profiles/closure_bench.json and prints it: per workload the device call (Engine.tdoa_closure_dev with all four outputs
in HBM, then synchronize; best of `repeats` after a warm-up call), the kernel times of pal_profile, the NumPy specification's time on the
same tables (closure.tdoa_closure, checked equal to the device's outputs) and, for the 64-microphone tables, Engine.solve_positions_dev
in the same process: the solve the check feeds.  No speed is promised; those two are the yardsticks."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import RECORD, Engine, closure  # noqa: E402
from pyaudiolocalization_amd.engine import pair_list  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fs, L, c = 48000.0, 12000, cases.C_SOUND
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


def workload(frames, mics_n, with_solve):
    rng = np.random.default_rng([7, mics_n])
    mics = cases.fibonacci_sphere(mics_n, 0.5)
    pl = pair_list(mics_n)
    tables = np.zeros((frames, len(pl)), dtype=RECORD)
    sources = rng.uniform(-3, 3, (frames, 3)) + np.array([0, 0, 1.5])
    for f in range(frames):
        d = np.linalg.norm(mics - sources[f], axis=1)
        lag = np.rint((d[pl[:, 1]] - d[pl[:, 0]]) / c * fs).astype(np.int64)
        bad = rng.choice(len(pl), len(pl) // 10, replace=False)
        lag[bad] = rng.integers(-2400, 2401, bad.shape[0])
        tables[f]["k_sel"] = lag + (L - 1)
        tables[f]["snr"] = 1.0
    out = closure.empty_outputs(frames, mics_n)
    d_tab = eng.alloc(tables.nbytes)
    d_out = [eng.alloc(a.nbytes) for a in out]
    eng.upload(d_tab, tables)

    def call():
        eng.tdoa_closure_dev(d_tab, frames, mics_n, L, 1, 1, "soft", *d_out)
        eng.synchronize()

    best = best_of(call)
    eng.profile_begin()
    call()
    eng.profile_end()
    kernels = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in eng.profile_entries().items() if k.startswith("k_closure")}
    for a, d in zip(out, d_out):
        eng.download(a, d)
    t0 = time.perf_counter()
    want = closure.tdoa_closure(tables["k_sel"], L, mics_n, 1, 1, "soft")
    spec_s = time.perf_counter() - t0
    equal = all(a.tobytes() == w.tobytes() for a, w in zip(out, want))
    res = {"frames": frames, "mics": mics_n, "pairs": len(pl), "triangle_tests_per_frame": len(pl) * (mics_n - 2), "repeats": repeats,
           "device_seconds_per_call": round(best, 6), "frames_per_s": round(frames / best, 1), "kernels": kernels,
           "numpy_specification_seconds": round(spec_s, 4), "device_equals_specification": bool(equal),
           "closed_triangles_mean": float(np.mean(out[3]["closed"])), "kept_pairs_mean": float(np.mean(out[3]["kept_pairs"]))}
    if with_solve:
        for name, kw in (("solve_positions_dev_ones", {}), ("solve_positions_dev_closure", {"weights": "closure"})):
            sec = best_of(lambda: eng.solve_positions_dev(d_tab, frames, L, mics, fs, c, **kw))
            rec = eng.solve_positions_dev(d_tab, frames, L, mics, fs, c, **kw)
            res[name] = {"seconds_per_call": round(sec, 6), "median_distance_to_source_m": float(np.median(np.linalg.norm(rec["position"] - sources, axis=1)))}
    eng.free(d_tab)
    for d in d_out:
        eng.free(d)
    return res


result = {"workloads": [workload(128, 64, True), workload(16, 256, False)]}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "closure_bench.json"), "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
eng.close()
