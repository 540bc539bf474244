#!/usr/bin/env python3
"""Bootstrap significance of every microphone pair on ONE GPU (utils.py:183-216; `analyze_correlation=True`): 64 microphones x
44 100 samples (synthetic.metric_frames), all 2016 pairs, 1000 shuffles each - 2 016 000 PHAT correlations per frame.

    python tools/bench_bootstrap.py [mics=64] [shuffles=1000] [repeats=2]

Prints one JSON line: the device path (Engine.bootstrap_peaks: counter-based shuffles on the device, csrc/bootstrap.hip) in
correlations/s and seconds per frame (best of `repeats` after one warm-up call); the host path (utils.bootstrap_significance with
rng="numpy": NumPy shuffles, batches uploaded to the pair pipeline) timed on 2 pairs and extrapolated to all of them - labelled
as such; and a parity sample: a few (pair, shuffle) peaks against the oracle's PHAT of the NumPy-restated shuffle."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyaudiolocalization_amd.engine as E  # noqa: E402
from oracle import pal_oracle as O  # noqa: E402
from pyaudiolocalization_amd import Engine, synthetic, utils  # noqa: E402
from pyaudiolocalization_amd.bootstrap import shuffle_indices  # noqa: E402
from pyaudiolocalization_amd.engine import pair_list  # noqa: E402

mics = int(sys.argv[1]) if len(sys.argv) > 1 else 64
shuffles = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
L, fs, seed, host_pairs = 44100, 44100.0, 0, 2

eng = Engine(0)
E._default = eng
frames = synthetic.metric_frames(1, mics, L)[0]
pairs = pair_list(mics)
P = len(pairs)

eng.bootstrap_peaks(frames, pairs[:4], 16, seed=seed)                 # plan, scratch
best, peaks = None, None
for _ in range(repeats):
    t0 = time.perf_counter()
    peaks = eng.bootstrap_peaks(frames, pairs, shuffles, seed=seed)
    el = time.perf_counter() - t0
    best = el if best is None else min(best, el)

np.random.seed(1)
t0 = time.perf_counter()
for i, j in pairs[:host_pairs]:
    utils.bootstrap_significance(frames[i], frames[j], fs, num_bootstrap=shuffles)
host_per_pair = (time.perf_counter() - t0) / host_pairs

rng = np.random.default_rng(5)
sample = [(int(p), int(s)) for p, s in zip(rng.integers(0, P, 4), rng.integers(0, shuffles, 4))]
rel = []
for p, s in sample:
    i, j = (int(v) for v in pairs[p])
    want = float(np.max(O.phat_correlation(frames[i], frames[j][shuffle_indices(L, i, j, s, "permutation", 50, seed)])))
    rel.append(abs(float(peaks[p, s]) - want) / abs(want))

print(json.dumps({
    "workload": {"mics": mics, "pairs": P, "samples": L, "shuffles": shuffles, "mode": "permutation"},
    "device": {"seconds_per_frame": round(best, 4), "correlations_per_s": round(P * shuffles / best, 1),
               "repeats": repeats},
    "host_numpy_rng": {"seconds_per_pair_measured": round(host_per_pair, 4), "pairs_timed": host_pairs,
                       "seconds_per_frame_extrapolated": round(host_per_pair * P, 1)},
    "speedup_vs_host_extrapolated": round(host_per_pair * P / best, 1),
    "parity_sample": {"pair_shuffle": sample, "max_rel_err": max(rel), "all_within_1e-10": bool(max(rel) <= 1e-10)},
    "peak_quantiles": [float(np.percentile(peaks, q)) for q in (5, 50, 95)],
}))
eng.close()
