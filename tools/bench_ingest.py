#!/usr/bin/env python3
"""Recorded-audio ingest on ONE GPU (csrc/resample.hip, stream.recorded_tdoa_stream): 64 microphones x 10 s at 48 kHz, resampled to
44.1 kHz, frames of 1 s every 0.5 s (19 frames of 2016 pairs).

    python tools/bench_ingest.py [mics=64] [seconds=10] [repeats=3]

Every step is a child process of its own under its own time limit (the parent never opens the GPU), and a step that fails ends the
run - nothing more is started on the GPU after it:
  device : Engine.resample_dev alone on the uploaded recording (best of `repeats` after a warm-up call, the device synchronised);
  chain  : recorded_tdoa_stream - seconds per stage (the device synchronised at every stage boundary) and, in a run without
           those synchronisations, the whole chain in frames per second;
  host   : signal_processing.resample_kaiser_best on the same array on this machine's CPUs (rows split over up to 16 worker
           processes), and whether the device's output equals it bit for bit.
Writes one JSON line to profiles/ingest_bench.json and prints it."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS_IN, FS = 48000.0, 44100.0
LIMITS = {"device": 240, "chain": 480, "host": 420}     # seconds per step


def recording(mics: int, seconds: float) -> np.ndarray:
    """One common noise sequence, delayed per microphone by an integer lag that changes half-way, plus independent noise at 0.3."""
    rng = np.random.default_rng(11)
    t_in = int(seconds * FS_IN)
    common = rng.standard_normal(t_in + 256)
    lags = rng.integers(-100, 101, (mics, 2))
    half = t_in // 2
    rows = np.empty((mics, t_in))
    for i in range(mics):
        rows[i, :half] = common[128 + lags[i, 0]: 128 + lags[i, 0] + half]
        rows[i, half:] = common[128 + lags[i, 1] + half: 128 + lags[i, 1] + t_in]
    rows += 0.3 * rng.standard_normal((mics, t_in))
    return rows


def step_device(mics, seconds, repeats, scratch):
    from pyaudiolocalization_amd import Engine
    rows = recording(mics, seconds)
    eng = Engine(0)
    m, t_in = rows.shape
    t = int(t_in * (FS / FS_IN))
    d_in, d_out = eng.alloc(rows.nbytes), eng.alloc(m * t * 8)
    t0 = time.perf_counter()
    eng.upload(d_in, rows)
    eng.synchronize()
    upload = time.perf_counter() - t0
    eng.resample_dev(d_in, m, t_in, FS_IN, FS, d_out, t)      # warm-up: code object, filter table
    eng.synchronize()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.resample_dev(d_in, m, t_in, FS_IN, FS, d_out, t)
        eng.synchronize()
        runs.append(time.perf_counter() - t0)
    eng.profile_begin()
    eng.resample_dev(d_in, m, t_in, FS_IN, FS, d_out, t)
    eng.synchronize()
    eng.profile_end()
    kernel_ms = eng.profile_entries().get("k_resample", (None, 0))[0]
    out = np.empty((m, t))
    eng.download(out, d_out)
    np.save(os.path.join(scratch, "device.npy"), out)
    eng.free(d_in); eng.free(d_out)
    eng.close()
    return {"upload_seconds": round(upload, 6), "resample_seconds": [round(r, 6) for r in runs], "resample_seconds_best": round(min(runs), 6),
            "k_resample_ms": None if kernel_ms is None else round(kernel_ms, 4), "output_samples_per_row": t}


def step_chain(mics, seconds, repeats, scratch):
    from pyaudiolocalization_amd import Engine
    from pyaudiolocalization_amd.stream import frame_count, recorded_tdoa_stream
    rows = recording(mics, seconds)
    eng = Engine(0)
    frame_len, hop = int(FS), int(FS) // 2
    args = (rows, FS_IN, FS, frame_len, hop, "butterworth", 0.01)
    recorded_tdoa_stream(*args, engine=eng)                   # warm-up: transform plans of every synchronised length
    timings = {}
    t0 = time.perf_counter()
    tables, lengths = recorded_tdoa_stream(*args, engine=eng, timings=timings)
    staged_wall = time.perf_counter() - t0
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        recorded_tdoa_stream(*args, engine=eng)
        walls.append(time.perf_counter() - t0)
    eng.close()
    frames = frame_count(int(rows.shape[1] * (FS / FS_IN)), frame_len, hop)
    total = sum(timings.values())
    return {"frames": frames, "pairs_per_frame": int(tables.shape[1]), "distinct_lengths": len(set(int(v) for v in lengths)),
            "stage_seconds": {k: round(v, 6) for k, v in timings.items()}, "stage_seconds_total": round(total, 6),
            "resample_share_of_stages": round(timings.get("resample", 0.0) / total, 4), "wall_seconds_with_stage_syncs": round(staged_wall, 6),
            "wall_seconds": [round(w, 6) for w in walls], "frames_per_s": round(frames / min(walls), 2)}


def _host_rows(rows):
    from pyaudiolocalization_amd.signal_processing import resample_kaiser_best
    return resample_kaiser_best(rows, FS_IN, FS)


def step_host(mics, seconds, repeats, scratch):
    import multiprocessing as mp
    rows = recording(mics, seconds)
    workers = min(16, os.cpu_count() or 1, mics)
    parts = np.array_split(rows, workers)
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(workers) as pool:        # (no process here has opened the GPU)
        out = np.concatenate(pool.map(_host_rows, parts))
    el = time.perf_counter() - t0
    dev_path = os.path.join(scratch, "device.npy")
    same = bool(np.array_equal(np.load(dev_path), out)) if os.path.exists(dev_path) else None
    return {"resample_kaiser_best_seconds": round(el, 3), "worker_processes": workers, "device_output_bit_identical": same}


STEPS = {"device": step_device, "chain": step_chain, "host": step_host}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, mics, seconds, repeats, scratch = sys.argv[2], int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
        print("RESULT " + json.dumps(STEPS[name](mics, seconds, repeats, scratch)))
        return 0
    mics = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = {"workload": {"mics": mics, "seconds": seconds, "fs_in": FS_IN, "fs": FS, "frame_seconds": 1.0, "hop_seconds": 0.5}}
    scratch = tempfile.mkdtemp(prefix="ingest_bench_")
    status = 0
    try:
        for name in ("device", "chain", "host"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, str(mics), str(seconds), str(repeats), scratch]
            try:
                run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
            except subprocess.TimeoutExpired:
                out[name] = {"error": f"no result within {LIMITS[name]} s"}
                status = 1
                break
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                out[name] = {"error": f"exit status {run.returncode}", "stderr_tail": run.stderr[-600:]}
                status = 1
                break
            out[name] = json.loads(lines[-1][len("RESULT "):])
            print(f"[bench_ingest] {name}: {lines[-1]}", file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    if status == 0:
        out["host_over_device_resample"] = round(out["host"]["resample_kaiser_best_seconds"] / out["device"]["resample_seconds_best"], 1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ingest_bench.json"), "w") as fh:
        fh.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    return status


if __name__ == "__main__":
    sys.exit(main())
