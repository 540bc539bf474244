#!/usr/bin/env python3
"""Delay-and-sum beamformer on ONE GPU (csrc/beamform.hip): 128 frames x 64 microphones x 12 000 samples at 48 kHz (the frame shape of
configuration C5) and 16 x 64 x 44 100 at 44.1 kHz, each steered at S = 1, 4 and 8 points per frame.

    python tools/bench_beamform.py [window_seconds=1] [compose_frames=2]

Writes one JSON to profiles/beamform_bench.json and prints it.  Per shape and S, on buffers resident in HBM (pal_steer_sum_dev):
- ms per call: after a warm-up call, as many calls as fill `window_seconds`, the device synchronised before and after the window;
- beams/s, and bytes/s on the compulsory bytes (frames read once, beams written once);
- pal_profile's times of the three parts of one call - the forward spectra, k_steer_sum, the inverse transforms - and which dominates;
- k_steer_sum alone beside its two floors from the shapes: its spectrum bytes (every spectrum once per pass of up to 8 beams, the beam
  spectra written once) over the 6.29 TB/s that a copy reaches on this device, and its M * S * H sincos evaluations, shown as a rate.
- the same beams composed the old way - Engine.fractional_delay on the S * M rows of a frame, then a host sum - on `compose_frames`
  frames, alternated with Engine.steer (the host form, so both sides pay their transfers) on the same frames in the same run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import Engine, beamform  # noqa: E402

window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
compose_frames = int(sys.argv[2]) if len(sys.argv) > 2 else 2
COPY_BYTES_PER_S = 6.29e12
SHAPES = ((128, 64, 12000, 48000.0), (16, 64, 44100, 44100.0))
BEAMS = (1, 4, 8)
c = cases.C_SOUND

eng = Engine(0)
rng = np.random.default_rng(12)
rows_out = []
for B, M, L, fs in SHAPES:
    mics = cases.fibonacci_sphere(M, 0.5)
    x = rng.standard_normal((B, M, L))
    d_x = eng.alloc(x.nbytes)
    eng.upload(d_x, x)
    H = L + 1
    for S in BEAMS:
        points = rng.uniform(-2.5, 2.5, (B, S, 3)) + np.array([0, 0, 1.5])
        delays, valid = beamform.point_delays(points, mics, c)
        weights = beamform.uniform_weights(valid, M)
        d_d, d_w, d_out = eng.alloc(delays.nbytes), eng.alloc(weights.nbytes), eng.alloc(B * S * L * 8)
        eng.upload(d_d, delays)
        eng.upload(d_w, weights)

        def call():
            eng.steer_dev(d_x, B, M, L, fs, d_d, d_w, S, d_out)

        call()
        eng.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            call()
            n += 1
            if n % 4 == 0 or n == 1:
                eng.synchronize()
                if time.perf_counter() - t0 >= window:
                    break
        eng.synchronize()
        per_call = (time.perf_counter() - t0) / n
        eng.profile_begin()
        call()
        eng.synchronize()
        eng.profile_end()
        prof = eng.profile_entries()
        parts = {k: round(prof.get(k, (0.0, 0))[0], 4) for k in ("steer_forward_spectra", "k_steer_sum", "steer_inverse")}
        t_sum = parts["k_steer_sum"] / 1e3
        passes = (S + 7) // 8
        sum_bytes = B * (passes * M + S) * H * 16
        compulsory = (B * M * L + B * S * L) * 8
        rows_out.append({
            "frames": B, "mics": M, "length": L, "fs": fs, "beams_per_frame": S, "calls_in_window": n,
            "ms_per_call": round(per_call * 1e3, 4), "beams_per_s": round(B * S / per_call, 1),
            "compulsory_bytes": compulsory, "compulsory_bytes_per_s": round(compulsory / per_call, 1),
            "parts_ms": parts, "dominant_part": max(parts, key=parts.get),
            "k_steer_sum": {"ms": parts["k_steer_sum"], "spectrum_bytes": sum_bytes,
                            "floor_ms_bytes_at_copy_rate": round(sum_bytes / COPY_BYTES_PER_S * 1e3, 4),
                            "bytes_per_s": round(sum_bytes / t_sum, 1) if t_sum else None,
                            "sincos_evaluations": B * M * S * H,
                            "sincos_per_s": round(B * M * S * H / t_sum, 1) if t_sum else None}})
        for p in (d_d, d_w, d_out):
            eng.free(p)
    # the composition the engine offered before: S * M delayed rows per frame through fractional_delay, summed on the host
    S = 4
    Bc = min(compose_frames, B)
    points = rng.uniform(-2.5, 2.5, (Bc, S, 3)) + np.array([0, 0, 1.5])
    delays, valid = beamform.point_delays(points, mics, c)
    weights = beamform.uniform_weights(valid, M)

    def composed():
        out = np.empty((Bc, S, L))
        for b in range(Bc):
            rows = np.broadcast_to(x[b][None], (S, M, L)).reshape(S * M, L)
            delayed = eng.fractional_delay(rows, delays[b].reshape(-1), fs).reshape(S, M, L)
            out[b] = np.einsum("sm,sml->sl", weights[b], delayed)
        return out

    def fused():
        return eng.steer(x[:Bc], fs, delays, weights)

    want, got = composed(), fused()
    t_comp, t_fused = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        composed()
        t_comp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        fused()
        t_fused.append(time.perf_counter() - t0)
    rows_out.append({"frames": Bc, "mics": M, "length": L, "fs": fs, "beams_per_frame": S, "host_forms": True,
                     "composed_fractional_delay_plus_host_sum_ms": round(min(t_comp) * 1e3, 3), "steer_ms": round(min(t_fused) * 1e3, 3),
                     "composed_over_steer": round(min(t_comp) / min(t_fused), 2),
                     "max_abs_difference": float(np.max(np.abs(want - got)))})
    eng.free(d_x)

out = {"window_seconds": window, "copy_bytes_per_s": COPY_BYTES_PER_S, "rows": rows_out}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "beamform_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
eng.close()
