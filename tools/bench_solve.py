#!/usr/bin/env python3
"""Batched device position solve on ONE GPU (main.py:233-298; csrc/solve.hip): 128 frames x 64 microphones on a sphere of 0.5 m (2016 pairs each,
synthetic sources + 20 us timing noise on the lag grid), 65 starts per frame.

    python tools/bench_solve.py [frames=128] [mics=64] [repeats=5] [host_frames=2] [--loss NAME --f-scale X]

Writes one JSON to profiles/solve_bench.json and prints it: the device path (Engine.solve_positions_dev on tables resident in HBM) in
positions/s (best of `repeats` after a warm-up call) with the kernel times of pal_profile; the host solve_position timed on
`host_frames` of the same tables on the same machine; and the largest distance between the two answers on those frames.

With --loss (soft_l1, huber or cauchy; --f-scale in metres, default 0.05) it instead times the linear loss and that loss on the same
tables in one process and writes both times, the mean trial points of the winners and the converged counts to
profiles/solve_robust_bench.json; the linear time of that run is the yardstick for the ratio."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import RECORD, Engine, solve  # noqa: E402
from pyaudiolocalization_amd.engine import pair_list  # noqa: E402
from pyaudiolocalization_amd.main import host_position  # noqa: E402

argv, loss, f_scale = [], None, 0.05
it = iter(sys.argv[1:])
for arg in it:
    if arg == "--loss":
        loss = next(it)
    elif arg == "--f-scale":
        f_scale = float(next(it))
    else:
        argv.append(arg)
if loss is not None:
    solve.check_loss(loss, f_scale)
frames = int(argv[0]) if len(argv) > 0 else 128
mics_n = int(argv[1]) if len(argv) > 1 else 64
repeats = int(argv[2]) if len(argv) > 2 else 5
host_frames = int(argv[3]) if len(argv) > 3 else 2
fs, L, c = 48000.0, 12000, cases.C_SOUND

rng = np.random.default_rng(7)
mics = cases.fibonacci_sphere(mics_n, 0.5)              # not planar: no mirror minimum, the error against the source means something
pl = pair_list(mics_n)
tables = np.zeros((frames, len(pl)), dtype=RECORD)
sources = rng.uniform(-3, 3, (frames, 3)) + np.array([0, 0, 1.5])
for f in range(frames):
    d = np.linalg.norm(mics - sources[f], axis=1)
    td = (d[pl[:, 1]] - d[pl[:, 0]]) / c + rng.normal(0, 2e-5, len(pl))
    tables[f]["k_sel"] = np.rint(td * fs).astype(np.int64) + (L - 1)
    tables[f]["snr"] = rng.uniform(2, 20, len(pl))

eng = Engine(0)
d_tab = eng.alloc(tables.nbytes)
eng.upload(d_tab, tables)


def timed(**kw):
    """-> (best seconds of `repeats` calls after a warm-up call, records, kernel times)."""
    eng.solve_positions_dev(d_tab, frames, L, mics, fs, c, **kw)
    best, rec = None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        rec = eng.solve_positions_dev(d_tab, frames, L, mics, fs, c, **kw)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    eng.profile_begin()
    eng.solve_positions_dev(d_tab, frames, L, mics, fs, c, **kw)
    eng.profile_end()
    return best, rec, {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in eng.profile_entries().items() if k.startswith("k_solve")}


if loss is not None:
    out = {"workload": {"frames": frames, "mics": mics_n, "pairs": len(pl), "starts": 1 + solve.GRID ** 3, "max_iter": solve.MAX_ITER,
                        "f_scale": f_scale, "repeats": repeats}}
    for name, kw in (("linear", {}), (loss, {"loss": loss, "f_scale": f_scale})):
        best, rec, kernels = timed(**kw)
        out[name] = {"seconds_per_call": round(best, 6), "positions_per_s": round(frames / best, 1), "kernels": kernels,
                     "converged_frames": int(np.count_nonzero(rec["status"] & solve.ST_CONVERGED)),
                     "trial_points_of_winner_mean": float(np.mean(rec["iterations"])),
                     "converged_starts_mean": float(np.mean(rec["converged_starts"])),
                     "max_abs_error_vs_source_m": float(np.max(np.abs(rec["position"] - sources)))}
    out["seconds_ratio_to_linear"] = round(out[loss]["seconds_per_call"] / out["linear"]["seconds_per_call"], 3)
    eng.free(d_tab)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "solve_robust_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    eng.close()
    sys.exit(0)

rec = eng.solve_positions_dev(d_tab, frames, L, mics, fs, c)          # warm-up: code objects, scratch, index table
best = None
for _ in range(repeats):
    t0 = time.perf_counter()
    rec = eng.solve_positions_dev(d_tab, frames, L, mics, fs, c)
    el = time.perf_counter() - t0
    best = el if best is None else min(best, el)
eng.profile_begin()
eng.solve_positions_dev(d_tab, frames, L, mics, fs, c)
eng.profile_end()
kernels = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in eng.profile_entries().items() if k.startswith("k_solve")}
eng.free(d_tab)

host_s, dist = [], []
for f in range(min(host_frames, frames)):
    t0 = time.perf_counter()
    pos = host_position(tables[f], L, mics, fs, c, None, "ones")
    host_s.append(time.perf_counter() - t0)
    dist.append(float(np.max(np.abs(pos - rec["position"][f]))))

out = {
    "workload": {"frames": frames, "mics": mics_n, "pairs": len(pl), "starts": 1 + solve.GRID ** 3, "max_iter": solve.MAX_ITER},
    "device": {"seconds_per_call": round(best, 6), "positions_per_s": round(frames / best, 1), "repeats": repeats, "kernels": kernels,
               "converged_frames": int(np.count_nonzero(rec["status"] & solve.ST_CONVERGED)),
               "trial_points_of_winner_mean": float(np.mean(rec["iterations"])),
               "max_abs_error_vs_source_m": float(np.max(np.abs(rec["position"] - sources)))},
    "host_solve_position": {"seconds_per_frame": [round(s, 3) for s in host_s], "frames_timed": len(host_s),
                            "max_abs_distance_to_device_m": max(dist) if dist else None},
    "speedup_per_frame": round(float(np.mean(host_s)) / (best / frames), 1) if host_s else None,
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "solve_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
eng.close()
