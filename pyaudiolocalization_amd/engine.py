"""Python face of one libpal_hip engine (one HIP device, one stream).

Host arrays in, host arrays out for the drop-in functions; ``*_dev`` methods work on buffers
that stay resident in HBM (``alloc`` / ``upload`` / ``download``).  All arithmetic happens in the
HIP kernels behind the C ABI - nothing here computes a result on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _ffi, bootstrap, closure, consensus, solve
from ._ffi import RECORD, PalError, PhatParams, SolveParams, f64, ptr


def _method_code(threshold_method: str) -> int:
    # utils.py:144-149: 'adaptive' is the only alternative, every other string means 'median'
    return 1 if threshold_method == "adaptive" else 0


def make_params(fs, num_peaks=1, threshold_method="median", threshold_multiplier=1.0,
                max_expected_delay=None) -> PhatParams:
    p = PhatParams()
    p.fs = float(fs)
    p.threshold_multiplier = float(threshold_multiplier)
    p.max_expected_delay = math.nan if max_expected_delay is None else float(max_expected_delay)
    p.threshold_method = _method_code(threshold_method)
    p.peak_distance = int(fs * 0.001)                       # utils.py:151
    p.num_peaks = int(num_peaks)
    p.reserved = 0
    return p


def pair_list(mics: int) -> np.ndarray:
    """(P, 2) mic indices in the row-major i<j order of main.py:202-203."""
    i, j = np.triu_indices(mics, k=1)
    return np.stack([i, j], axis=1).astype(np.int32)


class Engine:
    def __init__(self, device: Optional[int] = None):
        self._lib = _ffi.load()
        if device is None:
            device = int(os.environ.get("PAL_DEVICE", "0"))
        h = C.c_void_p()
        rc = self._lib.pal_create(int(device), C.byref(h))
        if rc != 0:
            text = self._lib.pal_last_error(None).decode()
            raise PalError(rc, f"pal_create(device={device}): {text} - the HIP engine needs an AMD GPU; "
                               "there is no CPU fallback")
        self._h = h
        self.device = int(device)

    # ---- plumbing -------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc == 0:
            return
        text = self._lib.pal_last_error(self._h).decode()
        if rc == _ffi.ERR_INVALID:
            raise ValueError(text)
        if rc == _ffi.ERR_NOMEM:
            raise MemoryError(text)
        raise PalError(rc, text)

    def synchronize(self) -> None:
        self._check(self._lib.pal_synchronize(self._h))

    def set_chunk(self, chunk: int) -> None:
        self._check(self._lib.pal_set_chunk(self._h, int(chunk)))

    def clear_plans(self) -> None:
        """Drop every cached transform plan (they are rebuilt on next use; the cache is bounded anyway)."""
        self._check(self._lib.pal_clear_plans(self._h))

    def set_max_plans(self, max_plans: int) -> None:
        """Bound of the plan caches (least recently used out first); see include/pal_hip.h."""
        self._check(self._lib.pal_set_max_plans(self._h, int(max_plans)))

    def plan_stats(self):
        """(plans built, plans evicted) since the engine was created."""
        b, e = C.c_int64(), C.c_int64()
        self._check(self._lib.pal_plan_stats(self._h, C.byref(b), C.byref(e)))
        return b.value, e.value

    def pair_group_size(self, length: int) -> int:
        """Packed transforms (two pairs each) per launch group of the all-pairs pipeline for frames of `length` samples."""
        g = C.c_int32()
        self._check(self._lib.pal_pair_group_size(self._h, int(length), C.byref(g)))
        return g.value

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.pal_device_alloc(self._h, int(nbytes), C.byref(p)))
        return int(p.value)

    def free(self, dptr: int) -> None:
        self._check(self._lib.pal_device_free(self._h, C.c_void_p(dptr)))

    def upload(self, dptr: int, host: np.ndarray) -> None:
        host = np.ascontiguousarray(host)
        self._check(self._lib.pal_upload(self._h, C.c_void_p(dptr), host.ctypes.data, host.nbytes))

    def download(self, host: np.ndarray, dptr: int) -> np.ndarray:
        assert host.flags.c_contiguous
        self._check(self._lib.pal_download(self._h, host.ctypes.data, C.c_void_p(dptr), host.nbytes))
        return host

    def plan_info(self, frame_len: int) -> dict:
        v = [C.c_int32() for _ in range(4)]
        self._check(self._lib.pal_plan_info(self._h, int(frame_len), *[C.byref(x) for x in v]))
        f = [C.c_int32() for _ in range(3)]
        self._check(self._lib.pal_plan_factors(self._h, int(frame_len), *[C.byref(x) for x in f]))
        return {"n": v[0].value, "conv_len": v[1].value, "m1": v[2].value, "m2": v[3].value,
                "n1": f[0].value, "n2": f[1].value, "tile_len": f[2].value}

    # ---- hot path A --------------------------------------------------------------------
    def gcc_phat_all_pairs(self, frames, fs, num_peaks=1, threshold_method="median", threshold_multiplier=1.0,
                           max_expected_delay=None, want_corr=False):
        """frames[B][M][L] (or [M][L]) -> TDOA table[B][P] (structured, see _ffi.RECORD) [+ corr[B][P][2L-1]]."""
        x = f64(frames)
        squeeze = x.ndim == 2
        if squeeze:
            x = x[None]
        if x.ndim != 3:
            raise ValueError("frames must be [M][L] or [B][M][L]")
        if num_peaks != 1:
            raise ValueError("the batched table carries one peak per pair (main.py:204 calls num_peaks=1)")
        b, m, length = x.shape
        npairs = m * (m - 1) // 2
        table = np.zeros((b, npairs), dtype=RECORD)
        corr = np.empty((b, npairs, 2 * length - 1)) if want_corr else None
        prm = make_params(fs, 1, threshold_method, threshold_multiplier, max_expected_delay)
        self._check(self._lib.pal_gcc_phat_all_pairs(self._h, x.ctypes.data, b, m, length, C.byref(prm),
                                                     table.ctypes.data, ptr(corr)))
        if squeeze:
            table = table[0]
            corr = None if corr is None else corr[0]
        return (table, corr) if want_corr else table

    def gcc_phat_all_pairs_dev(self, d_frames: int, b: int, m: int, length: int, prm: PhatParams, d_table: int) -> None:
        """Asynchronous: frames and table stay in HBM; call synchronize() before reading the table."""
        self._check(self._lib.pal_gcc_phat_all_pairs_dev(self._h, C.c_void_p(d_frames), b, m, length, C.byref(prm),
                                                         C.c_void_p(d_table)))

    def gcc_phat_all_pairs_peaks(self, frames, fs, num_peaks=4, threshold_method="median", threshold_multiplier=1.0, max_expected_delay=None):
        """frames[B][M][L] (or [M][L]) -> (table[B][P], cand_k[B][P][num_peaks] int32, cand_h[B][P][num_peaks]): the ordinary table (the
        records of the first peak) and the ``num_peaks`` (1 .. 8) selected peaks per pair, highest first: array indices (-1 past n_sel)
        and heights (+0.0 past n_sel) - the candidates of ``tdoa_consensus``."""
        x = f64(frames)
        squeeze = x.ndim == 2
        if squeeze:
            x = x[None]
        if x.ndim != 3:
            raise ValueError("frames must be [M][L] or [B][M][L]")
        k = int(num_peaks)
        if not 1 <= k <= _ffi.MAX_CANDIDATES:
            raise ValueError(f"num_peaks {k} outside 1..{_ffi.MAX_CANDIDATES}")
        b, m, length = x.shape
        npairs = m * (m - 1) // 2
        table = np.zeros((b, npairs), dtype=RECORD)
        cand_k = np.zeros((b, npairs, k), dtype=np.int32)
        cand_h = np.zeros((b, npairs, k), dtype=np.float64)
        prm = make_params(fs, k, threshold_method, threshold_multiplier, max_expected_delay)
        self._check(self._lib.pal_gcc_phat_all_pairs_peaks(self._h, x.ctypes.data, b, m, length, C.byref(prm), table.ctypes.data,
                                                           cand_k.ctypes.data, cand_h.ctypes.data))
        return (table[0], cand_k[0], cand_h[0]) if squeeze else (table, cand_k, cand_h)

    def gcc_phat_all_pairs_peaks_dev(self, d_frames: int, b: int, m: int, length: int, prm: PhatParams, d_table: int, d_cand_k: int,
                                     d_cand_h: int = 0) -> None:
        """Asynchronous: frames, table, cand_k[b][P][prm.num_peaks] (int32) and cand_h (float64; 0 = not wanted) stay in HBM."""
        if not 1 <= int(prm.num_peaks) <= _ffi.MAX_CANDIDATES:
            raise ValueError(f"num_peaks {int(prm.num_peaks)} outside 1..{_ffi.MAX_CANDIDATES}")
        self._check(self._lib.pal_gcc_phat_all_pairs_peaks_dev(self._h, C.c_void_p(d_frames), b, m, length, C.byref(prm), C.c_void_p(d_table),
                                                               C.c_void_p(d_cand_k), C.c_void_p(d_cand_h) if d_cand_h else None))

    def gcc_phat_pairs_peaks_dev(self, d_rows: int, r: int, length: int, d_pairs: int, p: int, prm: PhatParams, d_table: int, d_cand_k: int,
                                 d_cand_h: int = 0) -> None:
        """Asynchronous: as gcc_phat_pairs_dev, with cand_k[P][prm.num_peaks] and cand_h (0 = not wanted) in HBM."""
        if not 1 <= int(prm.num_peaks) <= _ffi.MAX_CANDIDATES:
            raise ValueError(f"num_peaks {int(prm.num_peaks)} outside 1..{_ffi.MAX_CANDIDATES}")
        self._check(self._lib.pal_gcc_phat_pairs_peaks_dev(self._h, C.c_void_p(d_rows), int(r), int(length), C.c_void_p(d_pairs), int(p),
                                                           C.byref(prm), C.c_void_p(d_table), C.c_void_p(d_cand_k),
                                                           C.c_void_p(d_cand_h) if d_cand_h else None))

    def gcc_phat_pairs(self, rows, pairs, fs, threshold_method="median", threshold_multiplier=1.0,
                       max_expected_delay=None) -> np.ndarray:
        """rows[R][L] and an explicit pair list pairs[P][2] (row indices) -> table[P]."""
        x = f64(rows)
        if x.ndim != 2:
            raise ValueError("rows must be [R][L]")
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        table = np.zeros(pr.shape[0], dtype=RECORD)
        prm = make_params(fs, 1, threshold_method, threshold_multiplier, max_expected_delay)
        self._check(self._lib.pal_gcc_phat_pairs(self._h, x.ctypes.data, x.shape[0], x.shape[1], pr.ctypes.data, pr.shape[0],
                                                 C.byref(prm), table.ctypes.data))
        return table

    def gcc_phat_pairs_dev(self, d_rows: int, r: int, length: int, d_pairs: int, p: int, prm: PhatParams, d_table: int) -> None:
        """Asynchronous: rows[R][L], pairs[P][2] (int32) and table[P] stay in HBM (a rank's block of a large frame's pair list)."""
        self._check(self._lib.pal_gcc_phat_pairs_dev(self._h, C.c_void_p(d_rows), int(r), int(length), C.c_void_p(d_pairs), int(p),
                                                     C.byref(prm), C.c_void_p(d_table)))

    # ---- bootstrap significance (utils.py:183-216; generator: bootstrap.py) -------------------
    def bootstrap_peaks(self, rows, pairs, num_bootstrap=1000, mode="permutation", block_size=50, seed=0) -> np.ndarray:
        """rows[R][L], pairs[P][2] -> peaks[P][num_bootstrap]: max PHAT(rows[i], shuffle s of rows[j]), shuffles keyed on
        (seed, i, j, s) (bootstrap.shuffle_indices)."""
        code = bootstrap.check_args(mode, block_size, num_bootstrap)
        x = f64(rows)
        if x.ndim != 2:
            raise ValueError("rows must be [R][L]")
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        peaks = np.empty((pr.shape[0], int(num_bootstrap)))
        self._check(self._lib.pal_bootstrap_peaks(self._h, x.ctypes.data, x.shape[0], x.shape[1], pr.ctypes.data, pr.shape[0],
                                                  int(num_bootstrap), code, int(block_size), int(seed), peaks.ctypes.data))
        return peaks

    def bootstrap_shuffle_dev(self, d_row: int, length: int, i: int, j: int, mode, block_size: int, seed: int, s0: int, count: int,
                              d_out: int) -> None:
        """Asynchronous: shuffles s0 .. s0+count-1 of the row d_row[length] under the key (seed, i, j) -> d_out[count][length]."""
        code = bootstrap.check_args(mode, block_size, count)
        self._check(self._lib.pal_bootstrap_shuffle_dev(self._h, C.c_void_p(d_row), int(length), int(i), int(j), code, int(block_size),
                                                        int(seed), int(s0), int(count), C.c_void_p(d_out)))

    def bootstrap_peaks_dev(self, d_rows: int, r: int, length: int, d_pairs: int, p: int, num_bootstrap: int, mode, block_size: int,
                            seed: int, d_peaks: int) -> None:
        """Asynchronous: rows[R][L], pairs[P][2] (int32) and peaks[P][num_bootstrap] stay in HBM."""
        code = bootstrap.check_args(mode, block_size, num_bootstrap)
        self._check(self._lib.pal_bootstrap_peaks_dev(self._h, C.c_void_p(d_rows), int(r), int(length), C.c_void_p(d_pairs), int(p),
                                                      int(num_bootstrap), code, int(block_size), int(seed), C.c_void_p(d_peaks)))

    # ---- position solve (main.py:233-298; algorithm: solve.py) ----------------------------------
    def _solve_args(self, nframes, npairs, lengths, mic_positions, fs, c, calib_delays, weights, buffer, grid, max_iter, extra_starts):
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        m = mics.shape[0]
        if m >= 2 and npairs != m * (m - 1) // 2:
            raise ValueError(f"a table of {m} microphones has {m * (m - 1) // 2} rows per frame, got {npairs}")
        ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.int32), (nframes,)))
        cal = None if calib_delays is None else f64(calib_delays, (m,))
        wt = None
        if isinstance(weights, str):
            if weights not in ("ones", "snr"):
                raise ValueError("weights: 'ones', 'snr', 'closure' or an array of [B][P] weights")
            mode = solve.WEIGHTS[weights]
        else:
            mode = solve.WEIGHTS["array"]
            wt = f64(weights).reshape(nframes, npairs)
        ex = None if extra_starts is None else f64(extra_starts).reshape(nframes, -1, 3)
        prm = SolveParams(float(fs), float(c), float(buffer), int(grid), int(max_iter), mode, 0 if ex is None else ex.shape[1])
        return m, ln, mics, cal, wt, ex, prm

    # ---- loop closure of TDOA tables (specification: closure.py) ---------------------------------
    def tdoa_closure(self, tables, lengths, m: int, tol: int = 1, min_votes: int = 1, mode: str = "soft", outputs=closure.OUTPUTS):
        """tables[B][P] (or [P]) of _ffi.RECORD, lengths[B] (or one length), m microphones -> (votes[B][P] int32, mic_closed[B][m] int32,
        weights[B][P] float64, summary[B] of closure.SUMMARY): per pair the third microphones whose triangle closes within ``tol``
        samples, per microphone its closed triangles, per pair the weight (``mode`` 'mask': 1 from ``min_votes`` votes, 'soft':
        votes / (m - 2) from ``min_votes`` votes, else 0) and per frame the counts - see closure.py.  ``outputs``: the names of the
        outputs to compute; the others come back as None."""
        tab = np.ascontiguousarray(tables, dtype=RECORD)
        if tab.ndim == 1:
            tab = tab[None]
        if tab.ndim != 2:
            raise ValueError("tables must be [P] or [B][P]")
        b, p = tab.shape
        code, ln = closure.check_args(b, m, lengths, tol, min_votes, mode)
        if p != int(m) * (int(m) - 1) // 2:
            raise ValueError(f"a table of {int(m)} microphones has {int(m) * (int(m) - 1) // 2} rows per frame, got {p}")
        out = closure.empty_outputs(b, int(m), outputs)
        self._check(self._lib.pal_tdoa_closure(self._h, tab.ctypes.data, b, int(m), ln.ctypes.data, int(tol), int(min_votes), code,
                                               *[ptr(a) for a in out]))
        return out

    def tdoa_closure_dev(self, d_tables: int, b: int, m: int, lengths, tol: int = 1, min_votes: int = 1, mode: str = "soft", d_votes: int = 0,
                         d_mic_closed: int = 0, d_weights: int = 0, d_summary: int = 0) -> None:
        """Asynchronous: tables[b][P] and the requested outputs (0 = not wanted; at least one) stay in HBM; ``lengths`` is read before
        the call returns.  A record whose k_sel lies outside 0..2 length - 2 is reported by ``synchronize``."""
        code, ln = closure.check_args(b, m, lengths, tol, min_votes, mode)
        self._check(self._lib.pal_tdoa_closure_dev(self._h, C.c_void_p(d_tables), int(b), int(m), ln.ctypes.data, int(tol), int(min_votes), code,
                                                   *[C.c_void_p(int(d)) if d else None for d in (d_votes, d_mic_closed, d_weights, d_summary)]))

    def _closure_weights_dev(self, d_tables: int, b: int, m: int, lengths, tol, min_votes, mode) -> np.ndarray:
        """The closure weights[b][P] of tables in HBM: only the weights come down."""
        w = np.zeros((int(b), m * (m - 1) // 2), dtype=np.float64)
        d_w = self.alloc(w.nbytes)
        try:
            self.tdoa_closure_dev(d_tables, b, m, lengths, tol, min_votes, mode, d_weights=d_w)
            self.synchronize()
            self.download(w, d_w)
        finally:
            self.free(d_w)
        return w

    # ---- loop-closure consensus over several candidates per pair (specification: consensus.py) -----
    def tdoa_consensus(self, cand_k, lengths, m: int, tol: int = 1, rounds: int = 2, tables=None, cand_h=None, outputs=None):
        """cand_k[B][P][K] (or [P][K]) int32 array indices (-1 = absent), lengths[B] (or one length), m microphones -> (sel[B][P] int32,
        table_out[B][P] of _ffi.RECORD, summary[B] of consensus.SUMMARY): per pair the candidate the other pairs' candidates agree with
        (stage 0, then ``rounds`` Jacobi rounds at ``tol`` samples - see consensus.py).  ``tables``: the records that table_out copies
        (k_sel, sel_height - when ``cand_h[B][P][K]`` is given - and the PAL_BR_CONSENSUS bit are replaced); without them table_out is
        None.  ``outputs``: the names of the outputs to compute (default: all that the arguments allow); the others come back as None."""
        ck = np.ascontiguousarray(cand_k, dtype=np.int32)
        if ck.ndim == 2:
            ck = ck[None]
        if ck.ndim != 3:
            raise ValueError("cand_k must be [P][K] or [B][P][K]")
        b, p, k = ck.shape
        ln = consensus.check_args(b, m, k, lengths, tol, rounds)
        if p != int(m) * (int(m) - 1) // 2:
            raise ValueError(f"a table of {int(m)} microphones has {int(m) * (int(m) - 1) // 2} rows per frame, got {p}")
        tab = None if tables is None else np.ascontiguousarray(tables, dtype=RECORD).reshape(b, p)
        ch = None if cand_h is None else f64(cand_h).reshape(b, p, k)
        if outputs is None:
            outputs = tuple(name for name in consensus.OUTPUTS if name != "table_out" or tab is not None)
        if not outputs or any(name not in consensus.OUTPUTS for name in outputs):
            raise ValueError(f"outputs: at least one of {consensus.OUTPUTS}")
        if "table_out" in outputs and tab is None:
            raise ValueError("table_out needs the input tables")
        shapes = {"sel": ((b, p), np.int32), "table_out": ((b, p), RECORD), "summary": ((b,), consensus.SUMMARY)}
        out = tuple(np.zeros(*shapes[name]) if name in outputs else None for name in consensus.OUTPUTS)
        self._check(self._lib.pal_tdoa_consensus(self._h, ptr(tab), ck.ctypes.data, ptr(ch), b, int(m), k, ln.ctypes.data, int(tol), int(rounds),
                                                 *[ptr(a) for a in out]))
        return out

    def tdoa_consensus_dev(self, d_cand_k: int, b: int, m: int, k: int, lengths, tol: int = 1, rounds: int = 2, d_tables: int = 0,
                           d_cand_h: int = 0, d_sel: int = 0, d_table_out: int = 0, d_summary: int = 0) -> None:
        """Asynchronous: cand_k[b][P][k], the optional tables[b][P] / cand_h[b][P][k] and the requested outputs (0 = not wanted; at least
        one) stay in HBM; ``lengths`` is read before the call returns.  A candidate outside 0..2 length - 2, an absent candidate 0 or a
        gap in a pair's candidates is reported by ``synchronize``."""
        ln = consensus.check_args(b, m, k, lengths, tol, rounds)
        dev = [C.c_void_p(int(d)) if d else None for d in (d_tables, d_cand_k, d_cand_h, d_sel, d_table_out, d_summary)]
        self._check(self._lib.pal_tdoa_consensus_dev(self._h, dev[0], dev[1], dev[2], int(b), int(m), int(k), ln.ctypes.data, int(tol),
                                                     int(rounds), dev[3], dev[4], dev[5]))

    # ---- steered-response power map (specification: srp.py) ---------------------------------------
    def gcc_phat_all_pairs_strips(self, frames, fs, T: int, W: int = 0, threshold_method="median", threshold_multiplier=1.0,
                                  max_expected_delay=None, want_table=True):
        """frames[B][M][L] (or [M][L]) -> (strips[B][P][2T+1], table[B][P] or None): every pair's GCC-PHAT row around zero lag in the
        centred lag s = d_j - d_i (``strips[..][p][T + s]``), smoothed by a triangle of half-width ``W`` (0..32; 0: the samples
        themselves), and the ordinary one-peak table of the same rows - see srp.strips.  T >= 0, T + W <= L - 1."""
        x = f64(frames)
        squeeze = x.ndim == 2
        if squeeze:
            x = x[None]
        if x.ndim != 3:
            raise ValueError("frames must be [M][L] or [B][M][L]")
        b, m, length = x.shape
        npairs = m * (m - 1) // 2
        t, w = int(T), int(W)
        out = np.zeros((b, npairs, max(2 * t + 1, 1)), dtype=np.float64)
        table = np.zeros((b, npairs), dtype=RECORD) if want_table else None
        prm = make_params(fs, 1, threshold_method, threshold_multiplier, max_expected_delay)
        self._check(self._lib.pal_gcc_phat_all_pairs_strips(self._h, x.ctypes.data, b, m, length, C.byref(prm), t, w, ptr(table),
                                                            out.ctypes.data))
        if squeeze:
            out, table = out[0], None if table is None else table[0]
        return out, table

    def gcc_phat_all_pairs_strips_dev(self, d_frames: int, b: int, m: int, length: int, prm: PhatParams, T: int, W: int, d_strips: int,
                                      d_table: int = 0) -> None:
        """Asynchronous: frames[b][m][length], strips[b][P][2T+1] and the table (0 = not wanted) stay in HBM."""
        self._check(self._lib.pal_gcc_phat_all_pairs_strips_dev(self._h, C.c_void_p(d_frames), int(b), int(m), int(length), C.byref(prm),
                                                                int(T), int(W), C.c_void_p(d_table) if d_table else None,
                                                                C.c_void_p(d_strips)))

    @staticmethod
    def _srp_grid(lo, hi, count) -> _ffi.SrpGrid:
        lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
        count = np.asarray(count, dtype=np.int64).reshape(-1)
        if lo.shape != (3,) or hi.shape != (3,) or count.shape != (3,):
            raise ValueError("lo, hi and count have three entries each")
        if np.any(np.abs(count) >= 2 ** 31):
            raise ValueError("a cell count does not fit int32")
        g = _ffi.SrpGrid()
        for a in range(3):
            g.lo[a], g.hi[a], g.count[a] = float(lo[a]), float(hi[a]), int(count[a])
        g.reserved = 0
        return g

    @staticmethod
    def _srp_inputs(strips, mic_positions, pair_weights):
        st = f64(strips)
        if st.ndim == 2:
            st = st[None]
        if st.ndim != 3 or st.shape[2] % 2 != 1:
            raise ValueError("strips must be [P][2T+1] or [B][P][2T+1]")
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        b, p, _ = st.shape
        m = mics.shape[0]
        if m >= 2 and p != m * (m - 1) // 2:
            raise ValueError(f"strips of {m} microphones have {m * (m - 1) // 2} rows per frame, got {p}")
        return st, mics, None if pair_weights is None else f64(pair_weights).reshape(b, p)

    def srp_map(self, strips, mic_positions, fs, c, lo, hi, count, pair_weights=None, K: int = 0, R: int = 1,
                outputs=("power", "peaks", "summary")):
        """strips[B][P][2T+1] (or [P][2T+1]) -> (power[B][G], peaks[B][K] of _ffi.SRP_PEAK, summary[B] of _ffi.SRP_FRAME): the steered-
        response power of every cell of the grid ``count`` cells over the box ``lo .. hi`` (g = (ix * ny + iy) * nz + iz), optionally
        weighted per pair, the first ``K`` (0..8) peaks of each map within the neighbourhood radius ``R`` (1..4 cells) and the clipped
        terms - see srp.srp_map and srp.map_peaks.  ``outputs``: the names to compute; the others (and ``peaks`` when K = 0) are None."""
        st, mics, wt = self._srp_inputs(strips, mic_positions, pair_weights)
        b, _, width = st.shape
        m = mics.shape[0]
        grid = self._srp_grid(lo, hi, count)
        k = int(K)
        if any(name not in ("power", "peaks", "summary") for name in outputs):
            raise ValueError("outputs: 'power', 'peaks', 'summary'")
        cells = max(int(grid.count[0]), 0) * max(int(grid.count[1]), 0) * max(int(grid.count[2]), 0)
        big = not all(1 <= int(grid.count[a]) <= 1024 for a in range(3)) or cells > (1 << 24)      # the call refuses it
        power = np.zeros((b, 1 if big else cells), dtype=np.float64) if "power" in outputs else None
        peaks = np.zeros((b, k), dtype=_ffi.SRP_PEAK) if "peaks" in outputs and 0 < k <= _ffi.SRP_MAX_PEAKS else None
        summ = np.zeros(b, dtype=_ffi.SRP_FRAME) if "summary" in outputs else None
        self._check(self._lib.pal_srp_map(self._h, st.ctypes.data, b, m, (width - 1) // 2, mics.ctypes.data, float(fs), float(c),
                                          C.byref(grid), ptr(wt), k, int(R), ptr(power), ptr(peaks), ptr(summ)))
        return power, peaks, summ

    def srp_map_dev(self, d_strips: int, b: int, T: int, mic_positions, fs, c, lo, hi, count, d_pair_weights: int = 0, K: int = 0, R: int = 1,
                    d_power: int = 0, d_peaks: int = 0, d_summary: int = 0) -> None:
        """Asynchronous: strips[b][P][2T+1], the optional pair_weights[b][P] and the requested outputs (0 = not wanted; at least one)
        stay in HBM; ``mic_positions`` and the grid are read before the call returns."""
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        grid = self._srp_grid(lo, hi, count)
        dev = [C.c_void_p(int(d)) if d else None for d in (d_strips, d_pair_weights, d_power, d_peaks, d_summary)]
        self._check(self._lib.pal_srp_map_dev(self._h, dev[0], int(b), mics.shape[0], int(T), mics.ctypes.data, float(fs), float(c),
                                              C.byref(grid), dev[1], int(K), int(R), dev[2], dev[3], dev[4]))

    def srp_peaks(self, power, lo, hi, count, K: int = 1, R: int = 1):
        """power[B][nx][ny][nz] (or [nx][ny][nz], or [B][G]) -> (peaks[B][K] of _ffi.SRP_PEAK, summary[B] of _ffi.SRP_FRAME): the first
        ``K`` peaks of every map by the neighbourhood rule of radius ``R`` - see srp.map_peaks."""
        grid = self._srp_grid(lo, hi, count)
        cells = int(grid.count[0]) * int(grid.count[1]) * int(grid.count[2])
        pw = f64(power)
        ok = all(1 <= int(grid.count[a]) <= 1024 for a in range(3)) and cells <= (1 << 24)          # otherwise the call refuses the grid
        if ok:
            if pw.size % cells:
                raise ValueError("power does not hold whole maps of the grid")
            pw = pw.reshape(-1, cells)
        b = pw.shape[0] if ok else 1
        k = int(K)
        peaks = np.zeros((b, k if 0 < k <= _ffi.SRP_MAX_PEAKS else 1), dtype=_ffi.SRP_PEAK)
        summ = np.zeros(b, dtype=_ffi.SRP_FRAME)
        self._check(self._lib.pal_srp_peaks(self._h, pw.ctypes.data, b, C.byref(grid), k, int(R), peaks.ctypes.data, summ.ctypes.data))
        return peaks, summ

    def srp_peaks_dev(self, d_power: int, b: int, lo, hi, count, K: int, R: int, d_peaks: int, d_summary: int = 0) -> None:
        """Asynchronous: power[b][G], peaks[b][K] and the summary (0 = not wanted) stay in HBM."""
        grid = self._srp_grid(lo, hi, count)
        self._check(self._lib.pal_srp_peaks_dev(self._h, C.c_void_p(d_power) if d_power else None, int(b), C.byref(grid), int(K), int(R),
                                                C.c_void_p(d_peaks) if d_peaks else None, C.c_void_p(d_summary) if d_summary else None))

    def srp_zoom(self, strips, mic_positions, fs, c, seeds, half0, Z: int = 8, levels: int = 3, pair_weights=None):
        """strips[B][P][2T+1] (or [P][2T+1]) and seeds[B][K] (or [K]) of _ffi.SRP_PEAK, as srp_map returns its peaks -> out[B][K] of
        _ffi.SRP_ZOOM: a coarse-to-fine search around every seed, ``levels`` levels of ``Z``^3 cells, the first over the seed's position
        -+ ``half0[3]`` metres, each next one over the best cell and half of each neighbour, with the strip read at the fractional lag
        (linear interpolation) - see srp.zoom, which it equals byte for byte.  An absent seed (index -1) gives an absent record."""
        st, mics, wt = self._srp_inputs(strips, mic_positions, pair_weights)
        b, _, width = st.shape
        m = mics.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=_ffi.SRP_PEAK)
        if sd.size % b:
            raise ValueError("seeds must be [K] or [B][K]")
        sd = sd.reshape(b, -1)
        h0 = f64(half0).reshape(-1)
        if h0.shape != (3,):
            raise ValueError("half0 has three entries")
        out = np.zeros(sd.shape, dtype=_ffi.SRP_ZOOM)
        self._check(self._lib.pal_srp_zoom(self._h, st.ctypes.data, b, m, (width - 1) // 2, mics.ctypes.data, float(fs), float(c), ptr(wt),
                                           sd.ctypes.data, sd.shape[1], h0.ctypes.data, int(Z), int(levels), out.ctypes.data))
        return out

    def srp_zoom_dev(self, d_strips: int, b: int, T: int, mic_positions, fs, c, d_seeds: int, K: int, half0, Z: int, levels: int, d_out: int,
                     d_pair_weights: int = 0) -> None:
        """Asynchronous: strips[b][P][2T+1], seeds[b][K], the optional pair_weights[b][P] and out[b][K] stay in HBM; ``mic_positions``
        and ``half0`` are read before the call returns."""
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        h0 = f64(half0).reshape(-1)
        if h0.shape != (3,):
            raise ValueError("half0 has three entries")
        dev = [C.c_void_p(int(d)) if d else None for d in (d_strips, d_pair_weights, d_seeds, d_out)]
        self._check(self._lib.pal_srp_zoom_dev(self._h, dev[0], int(b), mics.shape[0], int(T), mics.ctypes.data, float(fs), float(c), dev[1],
                                               dev[2], int(K), h0.ctypes.data, int(Z), int(levels), dev[3]))

    # ---- the direction map (specification: srp.py, doa_*) ------------------------------------------
    @staticmethod
    def _srp_doa_grid(az, el, wrap):
        """-> (pal_srp_doa_grid, az[n_az][2], el[n_el][2]): the tables as the call reads them; their values are the call's to refuse."""
        az, el = f64(az), f64(el)
        if az.ndim != 2 or el.ndim != 2 or az.shape[1] != 2 or el.shape[1] != 2:
            raise ValueError("az must be [n_az][2] and el [n_el][2]: (cos, sin)")
        g = _ffi.SrpDoaGrid()
        g.n_az, g.n_el, g.wrap, g.reserved = az.shape[0], el.shape[0], int(bool(wrap)), 0
        return g, az, el

    def srp_doa(self, strips, mic_positions, fs, c, az, el, wrap=1, pair_weights=None, K: int = 0, R: int = 1,
                outputs=("power", "peaks", "summary")):
        """strips[B][P][2T+1] (or [P][2T+1]) -> (power[B][n_az * n_el], peaks[B][K] of _ffi.SRP_PEAK, summary[B] of _ffi.SRP_FRAME): the
        steered-response power of every direction of the grid given by the tables ``az[n_az][2]`` and ``el[n_el][2]`` of (cos, sin), as
        srp.doa_axes builds them (g = ia * n_el + ie), under the plane-wave model, optionally weighted per pair; the first ``K`` (0..8)
        peaks of each map within ``R`` (1..4) cells, azimuth taken mod n_az when ``wrap``, with the cells' directions in x, y, z; and the
        clipped terms - see srp.doa_map and srp.doa_peaks, which it equals byte for byte.  ``outputs``: as in srp_map."""
        st, mics, wt = self._srp_inputs(strips, mic_positions, pair_weights)
        grid, az, el = self._srp_doa_grid(az, el, wrap)
        b, k = st.shape[0], int(K)
        if any(name not in ("power", "peaks", "summary") for name in outputs):
            raise ValueError("outputs: 'power', 'peaks', 'summary'")
        big = not (1 <= grid.n_az <= _ffi.SRP_MAX_DOA_COUNT and 1 <= grid.n_el <= _ffi.SRP_MAX_DOA_COUNT)        # the call refuses it
        power = np.zeros((b, 1 if big else grid.n_az * grid.n_el), dtype=np.float64) if "power" in outputs else None
        peaks = np.zeros((b, k), dtype=_ffi.SRP_PEAK) if "peaks" in outputs and 0 < k <= _ffi.SRP_MAX_PEAKS else None
        summ = np.zeros(b, dtype=_ffi.SRP_FRAME) if "summary" in outputs else None
        self._check(self._lib.pal_srp_doa(self._h, st.ctypes.data, b, mics.shape[0], (st.shape[2] - 1) // 2, mics.ctypes.data, float(fs),
                                          float(c), C.byref(grid), az.ctypes.data, el.ctypes.data, ptr(wt), k, int(R), ptr(power), ptr(peaks),
                                          ptr(summ)))
        return power, peaks, summ

    def srp_doa_dev(self, d_strips: int, b: int, T: int, mic_positions, fs, c, az, el, wrap=1, d_pair_weights: int = 0, K: int = 0,
                    R: int = 1, d_power: int = 0, d_peaks: int = 0, d_summary: int = 0) -> None:
        """Asynchronous: strips[b][P][2T+1], the optional pair_weights[b][P] and the requested outputs (0 = not wanted; at least one)
        stay in HBM; ``mic_positions`` and the tables are read before the call returns."""
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        grid, az, el = self._srp_doa_grid(az, el, wrap)
        dev = [C.c_void_p(int(d)) if d else None for d in (d_strips, d_pair_weights, d_power, d_peaks, d_summary)]
        self._check(self._lib.pal_srp_doa_dev(self._h, dev[0], int(b), mics.shape[0], int(T), mics.ctypes.data, float(fs), float(c),
                                              C.byref(grid), az.ctypes.data, el.ctypes.data, dev[1], int(K), int(R), dev[2], dev[3], dev[4]))

    def srp_doa_peaks(self, power, az, el, wrap=1, K: int = 1, R: int = 1):
        """power[B][n_az][n_el] (or [n_az][n_el], or [B][G]) -> (peaks[B][K] of _ffi.SRP_PEAK, summary[B] of _ffi.SRP_FRAME): the first
        ``K`` peaks of every direction map by the wrapped neighbourhood rule of radius ``R`` - see srp.doa_peaks."""
        grid, az, el = self._srp_doa_grid(az, el, wrap)
        cells = grid.n_az * grid.n_el
        pw = f64(power)
        ok = 1 <= grid.n_az <= _ffi.SRP_MAX_DOA_COUNT and 1 <= grid.n_el <= _ffi.SRP_MAX_DOA_COUNT                # otherwise the call refuses the grid
        if ok:
            if pw.size % cells:
                raise ValueError("power does not hold whole maps of the grid")
            pw = pw.reshape(-1, cells)
        b = pw.shape[0] if ok else 1
        k = int(K)
        peaks = np.zeros((b, k if 0 < k <= _ffi.SRP_MAX_PEAKS else 1), dtype=_ffi.SRP_PEAK)
        summ = np.zeros(b, dtype=_ffi.SRP_FRAME)
        self._check(self._lib.pal_srp_doa_peaks(self._h, pw.ctypes.data, b, C.byref(grid), az.ctypes.data, el.ctypes.data, k, int(R),
                                                peaks.ctypes.data, summ.ctypes.data))
        return peaks, summ

    def srp_doa_peaks_dev(self, d_power: int, b: int, az, el, wrap, K: int, R: int, d_peaks: int, d_summary: int = 0) -> None:
        """Asynchronous: power[b][G], peaks[b][K] and the summary (0 = not wanted) stay in HBM."""
        grid, az, el = self._srp_doa_grid(az, el, wrap)
        self._check(self._lib.pal_srp_doa_peaks_dev(self._h, C.c_void_p(d_power) if d_power else None, int(b), C.byref(grid), az.ctypes.data,
                                                    el.ctypes.data, int(K), int(R), C.c_void_p(d_peaks) if d_peaks else None,
                                                    C.c_void_p(d_summary) if d_summary else None))

    def srp_doa_zoom(self, strips, mic_positions, fs, c, seeds, half0, Z: int = 8, levels: int = 3, pair_weights=None):
        """strips[B][P][2T+1] (or [P][2T+1]) and seeds[B][K] (or [K]) of _ffi.SRP_PEAK, as srp_doa returns its peaks -> out[B][K] of
        _ffi.SRP_ZOOM with the direction in x, y, z: the zoom on the sphere, ``levels`` levels of ``Z``^2 directions, the first over the
        seed's direction -+ ``half0`` (one number, radians for small values) in its tangent plane, each next one over the best cell and
        half of each neighbour - see srp.doa_zoom, which it equals byte for byte.  An absent seed (index -1) gives an absent record."""
        st, mics, wt = self._srp_inputs(strips, mic_positions, pair_weights)
        b = st.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=_ffi.SRP_PEAK)
        if sd.size % b:
            raise ValueError("seeds must be [K] or [B][K]")
        sd = sd.reshape(b, -1)
        if np.ndim(half0) != 0:
            raise ValueError("half0 is one number")
        out = np.zeros(sd.shape, dtype=_ffi.SRP_ZOOM)
        self._check(self._lib.pal_srp_doa_zoom(self._h, st.ctypes.data, b, mics.shape[0], (st.shape[2] - 1) // 2, mics.ctypes.data, float(fs),
                                               float(c), ptr(wt), sd.ctypes.data, sd.shape[1], float(half0), int(Z), int(levels),
                                               out.ctypes.data))
        return out

    def srp_doa_zoom_dev(self, d_strips: int, b: int, T: int, mic_positions, fs, c, d_seeds: int, K: int, half0, Z: int, levels: int,
                         d_out: int, d_pair_weights: int = 0) -> None:
        """Asynchronous: strips[b][P][2T+1], seeds[b][K], the optional pair_weights[b][P] and out[b][K] stay in HBM; ``mic_positions``
        is read before the call returns."""
        mics = f64(mic_positions)
        if mics.ndim != 2 or mics.shape[1] != 3:
            raise ValueError("mic_positions must be [M][3]")
        dev = [C.c_void_p(int(d)) if d else None for d in (d_strips, d_pair_weights, d_seeds, d_out)]
        self._check(self._lib.pal_srp_doa_zoom_dev(self._h, dev[0], int(b), mics.shape[0], int(T), mics.ctypes.data, float(fs), float(c),
                                                   dev[1], dev[2], int(K), float(half0), int(Z), int(levels), dev[3]))

    def solve_positions(self, tables, lengths, mic_positions, fs, c, calib_delays=None, weights="ones", buffer=5.0, grid=solve.GRID,
                        max_iter=solve.MAX_ITER, extra_starts=None, loss="linear", f_scale=1.0, return_pair_weights=False,
                        closure_tol=1, closure_min_votes=1, closure_mode="soft"):
        """tables[B][P] (or [P]) of _ffi.RECORD, lengths[B] (or one length) -> records[B] of solve.POSITION.  ``weights``: 'ones',
        'snr' (snr / mean(snr) of the records, as compute_weights), 'closure' or an array [B][P]; ``extra_starts`` [B][n][3].  ``loss``: one of
        solve.LOSSES, with ``f_scale`` in metres of weighted residual, for tables with outlier pairs; ``return_pair_weights``:
        -> (records, rho'(z)[B][P] at the positions: 1 for a pair the fit kept, towards 0 for one it discounted).
        ``weights='closure'``: the weights of ``tdoa_closure(tables, lengths, M, closure_tol, closure_min_votes, closure_mode)``, computed on
        the device, as the array.  A frame that keeps fewer than four pairs is solved like any other: its record means nothing, and
        ``kept_pairs`` of ``tdoa_closure``'s summary is where the caller sees it."""
        code, f_scale = solve.check_loss(loss, f_scale)
        tab = np.ascontiguousarray(tables, dtype=RECORD)
        if tab.ndim == 1:
            tab = tab[None]
        if tab.ndim != 2:
            raise ValueError("tables must be [P] or [B][P]")
        b, p = tab.shape
        if isinstance(weights, str) and weights == "closure":
            weights = self.tdoa_closure(tab, lengths, np.asarray(mic_positions).shape[0], closure_tol, closure_min_votes, closure_mode,
                                        outputs=("weights",))[2]
        m, ln, mics, cal, wt, ex, prm = self._solve_args(b, p, lengths, mic_positions, fs, c, calib_delays, weights, buffer, grid, max_iter,
                                                         extra_starts)
        out = np.zeros(b, dtype=solve.POSITION)
        if code == 0 and not return_pair_weights:
            self._check(self._lib.pal_solve_positions(self._h, tab.ctypes.data, b, m, ln.ctypes.data, mics.ctypes.data, ptr(cal), ptr(wt),
                                                      ptr(ex), C.byref(prm), out.ctypes.data))
            return out
        pw = np.zeros((b, p), dtype=np.float64) if return_pair_weights else None
        self._check(self._lib.pal_solve_positions_loss(self._h, tab.ctypes.data, b, m, ln.ctypes.data, mics.ctypes.data, ptr(cal), ptr(wt),
                                                       ptr(ex), C.byref(prm), out.ctypes.data, code, f_scale, ptr(pw)))
        return (out, pw) if return_pair_weights else out

    def solve_positions_dev(self, d_tables: int, b: int, lengths, mic_positions, fs, c, calib_delays=None, weights="ones", buffer=5.0,
                            grid=solve.GRID, max_iter=solve.MAX_ITER, extra_starts=None, loss="linear", f_scale=1.0,
                            return_pair_weights=False, closure_tol=1, closure_min_votes=1, closure_mode="soft"):
        """The same with the tables[B][P] in HBM (e.g. where gcc_phat_all_pairs_dev wrote them); returns when the records are on the host.
        ``weights='closure'``: the closure check runs on the tables where they are and only its weights come down, to go into the solve
        as the array (a frame that keeps fewer than four pairs is solved like any other: see solve_positions)."""
        code, f_scale = solve.check_loss(loss, f_scale)
        m = np.asarray(mic_positions).shape[0]
        if isinstance(weights, str) and weights == "closure":
            weights = self._closure_weights_dev(d_tables, b, m, lengths, closure_tol, closure_min_votes, closure_mode)
        m, ln, mics, cal, wt, ex, prm = self._solve_args(int(b), m * (m - 1) // 2, lengths, mic_positions, fs, c, calib_delays, weights, buffer,
                                                         grid, max_iter, extra_starts)
        out = np.zeros(int(b), dtype=solve.POSITION)
        if code == 0 and not return_pair_weights:
            self._check(self._lib.pal_solve_positions_dev(self._h, C.c_void_p(d_tables), int(b), m, ln.ctypes.data, mics.ctypes.data, ptr(cal),
                                                          ptr(wt), ptr(ex), C.byref(prm), out.ctypes.data))
            return out
        pw = np.zeros((int(b), m * (m - 1) // 2), dtype=np.float64) if return_pair_weights else None
        self._check(self._lib.pal_solve_positions_loss_dev(self._h, C.c_void_p(d_tables), int(b), m, ln.ctypes.data, mics.ctypes.data, ptr(cal),
                                                           ptr(wt), ptr(ex), C.byref(prm), out.ctypes.data, code, f_scale, ptr(pw)))
        return (out, pw) if return_pair_weights else out

    def phat_correlation(self, sig1, sig2) -> np.ndarray:
        a, b = f64(sig1), f64(sig2)
        if a.ndim != 1 or b.ndim != 1:
            raise ValueError("signals must be one-dimensional")
        corr = np.empty(a.shape[0] + b.shape[0] - 1)
        self._check(self._lib.pal_phat_correlation(self._h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0],
                                                   corr.ctypes.data))
        return corr

    def get_time_delays_phat(self, sig1, sig2, fs, num_peaks=1, threshold_method="median", threshold_multiplier=1.0,
                             max_expected_delay=None, want_corr=True):
        """-> (selected array indices k[<=num_peaks], record, corr)."""
        a, b = f64(sig1), f64(sig2)
        if a.ndim != 1 or b.ndim != 1:
            raise ValueError("signals must be one-dimensional")
        prm = make_params(fs, num_peaks, threshold_method, threshold_multiplier, max_expected_delay)
        ks = np.full(max(1, int(num_peaks)), -1, dtype=np.int32)
        rec = np.zeros(1, dtype=RECORD)
        corr = np.empty(a.shape[0] + b.shape[0] - 1) if want_corr else None
        self._check(self._lib.pal_get_time_delays_phat(self._h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0],
                                                       C.byref(prm), ks.ctypes.data, rec.ctypes.data, ptr(corr)))
        return ks[: int(rec["n_sel"][0])], rec[0], corr

    def corr_metrics(self, corr) -> np.void:
        c = f64(corr)
        rec = np.zeros(1, dtype=RECORD)
        self._check(self._lib.pal_corr_metrics(self._h, c.ctypes.data, c.shape[0], rec.ctypes.data))
        return rec[0]

    def select_peaks(self, rows, n2, fs, num_peaks=1, threshold_method="median", threshold_multiplier=1.0,
                     max_expected_delay=None):
        """Existing correlation rows[R][n] (or one row) with the lag mapping k - (n2 - 1) -> (table[R], k[R][num_peaks]);
        entries of k past a row's n_sel are -1."""
        x = f64(rows)
        if x.ndim == 1:
            x = x[None]
        if x.ndim != 2:
            raise ValueError("rows must be [n] or [R][n]")
        prm = make_params(fs, num_peaks, threshold_method, threshold_multiplier, max_expected_delay)
        table = np.zeros(x.shape[0], dtype=RECORD)
        ks = np.full((x.shape[0], max(1, int(num_peaks))), -1, dtype=np.int32)
        self._check(self._lib.pal_select_peaks(self._h, x.ctypes.data, x.shape[0], x.shape[1], int(n2), C.byref(prm),
                                               table.ctypes.data, ks.ctypes.data))
        return table, ks

    # ---- hot path B --------------------------------------------------------------------
    def simulate_multipath(self, base, fs, total_samples, delays, gains, trim_len=0) -> np.ndarray:
        """base[B][nbase], delays/gains[B][M][K] -> out[B][M][out_len] (normalised + compressed)."""
        x = f64(base)
        if x.ndim == 1:
            x = x[None]
        d, g = f64(delays), f64(gains)
        if d.ndim == 2:
            d, g = d[None], g[None]
        if d.shape != g.shape or d.ndim != 3 or d.shape[0] != x.shape[0]:
            raise ValueError("delays/gains must be [B][M][K] matching base[B][nbase]")
        b, m, k = d.shape
        out_len = trim_len if 0 < trim_len < total_samples else total_samples
        out = np.empty((b, m, out_len))
        self._check(self._lib.pal_simulate_multipath(self._h, x.ctypes.data, b, x.shape[1], float(fs), int(total_samples),
                                                     d.ctypes.data, g.ctypes.data, m, k, int(trim_len), out.ctypes.data))
        return out

    def fractional_delay(self, rows, delays, fs) -> np.ndarray:
        x = f64(rows)
        one = x.ndim == 1
        if one:
            x = x[None]
        d = f64(np.atleast_1d(delays))
        if d.shape != (x.shape[0],):
            raise ValueError("one delay per row")
        out = np.empty_like(x)
        self._check(self._lib.pal_fractional_delay(self._h, x.ctypes.data, x.shape[0], x.shape[1], d.ctypes.data, float(fs),
                                                   out.ctypes.data))
        return out[0] if one else out

    @staticmethod
    def _steer_tables(frames, delays, weights, default):
        """what steer and separate do to their arrays: -> x[B][M][L], d[B][S][M], w[B][S][M] (``default(m)`` where weights is None), one"""
        x, d = f64(frames), f64(delays)
        one = x.ndim == 2 and d.ndim == 2
        if one:
            x, d = x[None], d[None]
        if x.ndim != 3 or d.ndim != 3 or d.shape[0] != x.shape[0] or d.shape[2] != x.shape[1]:
            raise ValueError("frames must be [B][M][L] with delays[B][S][M] (or [M][L] with [S][M])")
        b, m, length = x.shape
        if weights is None:
            w = np.full(d.shape, default(m))
        else:
            w = f64(weights)
            if one and w.ndim == 2:
                w = w[None]
            if w.shape != d.shape:
                raise ValueError("weights must have the shape of delays")
        if m < 1 or d.shape[1] < 1 or b < 1:
            raise ValueError("need at least one frame, one microphone and one steering point")
        if length < 100:
            raise ValueError("steering needs at least 100 samples (the fade window of fractional_delay)")
        return x, d, w, one

    def steer(self, frames, fs, delays, weights=None) -> np.ndarray:
        """Delay-and-sum beams: frames[B][M][L], delays[B][S][M] (seconds) and weights[B][S][M] (None: 1/M) -> out[B][S][L]
        (rule: beamform.steer).  frames[M][L] with delays[S][M] gives out[S][L]."""
        x, d, w, one = self._steer_tables(frames, delays, weights, lambda m: 1.0 / m if m else 0.0)
        b, m, length = x.shape
        s = d.shape[1]
        out = np.empty((b, s, length))
        self._check(self._lib.pal_steer_sum(self._h, x.ctypes.data, b, m, length, float(fs), d.ctypes.data, w.ctypes.data, s,
                                            out.ctypes.data))
        return out[0] if one else out

    def separate(self, frames, fs, delays, gains=None, loading=0.01) -> np.ndarray:
        """Null-steering beams: frames[B][M][L], delays[B][S][M] (seconds) and gains[B][S][M] (None: 1) -> out[B][S][L], every beam
        with the other S - 1 sources cancelled (rule: beamform.separate).  S <= 8; loading >= 0, and > 0 where S > 1.  frames[M][L]
        with delays[S][M] gives out[S][L]."""
        x, d, g, one = self._steer_tables(frames, delays, gains, lambda m: 1.0)
        b, m, length = x.shape
        s = d.shape[1]
        out = np.empty((b, s, length))
        self._check(self._lib.pal_separate(self._h, x.ctypes.data, b, m, length, float(fs), d.ctypes.data, g.ctypes.data, s, float(loading),
                                           out.ctypes.data))
        return out[0] if one else out

    def separate_dev(self, d_frames: int, b: int, m: int, length: int, fs: float, d_delays: int, d_gains: int, s: int, loading: float,
                     d_out: int) -> None:
        """Engine.separate on buffers in HBM: d_frames[b][m][length], d_delays / d_gains[b][s][m] -> d_out[b][s][length]; asynchronous,
        refused table entries and non-finite samples surface in synchronize()."""
        self._check(self._lib.pal_separate_dev(self._h, C.c_void_p(d_frames), int(b), int(m), int(length), float(fs), C.c_void_p(d_delays),
                                               C.c_void_p(d_gains), int(s), float(loading), C.c_void_p(d_out)))

    def mvdr(self, frames, fs, delays, gains=None, loading=0.1, groups=1, return_weights=False):
        """MVDR beams: frames[B][M][L] in ``groups`` groups of B / groups consecutive frames, delays[G][S][M] (seconds) and
        gains[G][S][M] (None: 1) -> out[B][S][L] (rule: beamform.mvdr): the weights come from each group's own covariance under the
        diagonal loading ``loading * tr(R) / M``.  M <= 64, loading > 0.  delays[S][M] serves one group.  ``return_weights``: ->
        (out, w[G][S][M][L + 1] complex), the bins 0 .. L of beamform.mvdr_weights."""
        x, d = f64(frames), f64(delays)
        if d.ndim == 2:
            d = d[None]
        groups = int(groups)
        if x.ndim != 3 or d.ndim != 3 or d.shape[2] != x.shape[1]:
            raise ValueError("frames must be [B][M][L] with delays[G][S][M] (or [S][M] for one group)")
        b, m, length = x.shape
        if groups < 1 or b % groups or d.shape[0] != groups:
            raise ValueError("groups must be >= 1, divide the number of frames and count the steering tables")
        if gains is None:
            g = np.ones(d.shape)
        else:
            g = f64(gains)
            if g.ndim == 2:
                g = g[None]
            if g.shape != d.shape:
                raise ValueError("gains must have the shape of delays")
        s = d.shape[1]
        if m < 1 or s < 1 or b < 1:
            raise ValueError("need at least one frame, one microphone and one steering point")
        if length < 100:
            raise ValueError("steering needs at least 100 samples (the fade window of fractional_delay)")
        out = np.empty((b, s, length))
        w = np.empty((groups, s, m, length + 1), dtype=np.complex128) if return_weights else None
        self._check(self._lib.pal_mvdr(self._h, x.ctypes.data, b, m, length, float(fs), d.ctypes.data, g.ctypes.data, groups, s,
                                       float(loading), out.ctypes.data, w.ctypes.data if return_weights else None))
        return (out, w) if return_weights else out

    def mvdr_dev(self, d_frames: int, b: int, m: int, length: int, fs: float, d_delays: int, d_gains: int, groups: int, s: int,
                 loading: float, d_out: int, d_weights: int = 0) -> None:
        """Engine.mvdr on buffers in HBM: d_frames[b][m][length], d_delays / d_gains[groups][s][m] -> d_out[b][s][length] and, where
        d_weights is not 0, d_weights[groups][s][m][length + 1] complex; asynchronous, refused table entries and non-finite samples
        surface in synchronize()."""
        self._check(self._lib.pal_mvdr_dev(self._h, C.c_void_p(d_frames), int(b), int(m), int(length), float(fs), C.c_void_p(d_delays),
                                           C.c_void_p(d_gains), int(groups), int(s), float(loading), C.c_void_p(d_out),
                                           C.c_void_p(d_weights or None)))

    def steer_dev(self, d_frames: int, b: int, m: int, length: int, fs: float, d_delays: int, d_weights: int, s: int, d_out: int) -> None:
        """Engine.steer on buffers in HBM: d_frames[b][m][length], d_delays / d_weights[b][s][m] -> d_out[b][s][length]; asynchronous,
        refused table entries and non-finite samples surface in synchronize()."""
        self._check(self._lib.pal_steer_sum_dev(self._h, C.c_void_p(d_frames), int(b), int(m), int(length), float(fs), C.c_void_p(d_delays),
                                                C.c_void_p(d_weights), int(s), C.c_void_p(d_out)))

    def normalize_compress(self, rows, normalize_only=False, threshold=0.8, epsilon=1e-8) -> np.ndarray:
        x = f64(rows)
        one = x.ndim == 1
        if one:
            x = x[None]
        out = np.empty_like(x)
        self._check(self._lib.pal_normalize_compress(self._h, x.ctypes.data, x.shape[0], x.shape[1], int(normalize_only),
                                                     float(threshold), float(epsilon), out.ctypes.data))
        return out[0] if one else out

    def filtfilt(self, b, a, zi, rows) -> np.ndarray:
        x = f64(rows)
        one = x.ndim == 1
        if one:
            x = x[None]
        b, a, zi = f64(b), f64(a), f64(zi)
        out = np.empty_like(x)
        self._check(self._lib.pal_filtfilt(self._h, b.ctypes.data, b.shape[0], a.ctypes.data, a.shape[0], zi.ctypes.data,
                                           x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data))
        return out[0] if one else out

    def wiener3(self, rows) -> np.ndarray:
        x = f64(rows)
        one = x.ndim == 1
        if one:
            x = x[None]
        out = np.empty_like(x)
        self._check(self._lib.pal_wiener3(self._h, x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data))
        return out[0] if one else out

    def xcorr_vs_ref(self, rows, ref_idx: int):
        """Full cross-correlation of every row against row ref_idx -> (kpk[R], win5[R][5], pkabs[R], refpk)."""
        x = f64(rows)
        r = x.shape[0]
        kpk = np.zeros(r, dtype=np.int32)
        win = np.zeros((r, 5))
        pk = np.zeros(r)
        ref = C.c_double()
        self._check(self._lib.pal_xcorr_vs_ref(self._h, x.ctypes.data, r, x.shape[1], int(ref_idx), kpk.ctypes.data,
                                               win.ctypes.data, pk.ctypes.data, C.byref(ref)))
        return kpk, win, pk, ref.value

    # ---- device-resident stage chain (main.py:165-204 without host copies of the waveforms) ------
    def simulate_multipath_dev(self, d_base: int, b: int, nbase: int, fs: float, total_samples: int, d_delays: int, d_gains: int,
                               m: int, k: int, trim_len: int, d_out: int) -> None:
        self._check(self._lib.pal_simulate_multipath_dev(self._h, C.c_void_p(d_base), int(b), int(nbase), float(fs), int(total_samples),
                                                         C.c_void_p(d_delays), C.c_void_p(d_gains), int(m), int(k), int(trim_len),
                                                         C.c_void_p(d_out)))

    def row_energies_dev(self, d_rows: int, r: int, n: int) -> np.ndarray:
        """Sum of squares of every row of d_rows[r][n] (device summation order) -> energy[r] on the host."""
        en = np.zeros(r)
        self._check(self._lib.pal_row_energies_dev(self._h, C.c_void_p(d_rows), int(r), int(n), en.ctypes.data))
        return en

    def sync_measure_dev(self, d_rows: int, b: int, m: int, n: int):
        """Per frame: reference microphone (highest energy) and the cross-correlation measurements of every row against it
        -> (ref_idx[B], kpk[B][M], win5[B][M][5], pkabs[B][M], refpk[B]) on the host (a few numbers per row)."""
        # The reference microphone is np.argmax of np.sum(sig**2) (utils.py:413-414).  The device sums in another order: where the two
        # highest energies of a frame agree to 1e-12 (mirrored geometries, equal rows) those rows come to the host and numpy
        # itself decides, so that the choice - and with it every shift, pad and length behind it - is the reference's.
        en = self.row_energies_dev(d_rows, b * m, n).reshape(b, m)
        ref = np.full(b, -1, dtype=np.int32)
        for f in range(b):
            if not np.all(np.isfinite(en[f])):
                continue                                            # (NaN rows: the device's rule, as np.argmax)
            top = float(en[f].max())
            close = np.flatnonzero(en[f] >= top - 1e-12 * abs(top))
            if close.size > 1:
                exact = en[f].copy()
                row = np.empty(n)
                for q in close:
                    self.download(row, d_rows + (f * m + int(q)) * n * 8)
                    exact[q] = np.sum(row ** 2)
                exact[np.setdiff1d(np.arange(m), close)] = -np.inf
                ref[f] = int(np.argmax(exact))
        kpk = np.zeros((b, m), dtype=np.int32)
        win = np.zeros((b, m, 5))
        pk = np.zeros((b, m))
        refpk = np.zeros(b)
        self._check(self._lib.pal_sync_measure_dev(self._h, C.c_void_p(d_rows), int(b), int(m), int(n), ref.ctypes.data, kpk.ctypes.data,
                                                   win.ctypes.data, pk.ctypes.data, refpk.ctypes.data))
        return ref, kpk, win, pk, refpk

    def align_rows_dev(self, d_rows: int, r: int, n: int, pad_left, lout: int, d_out: int) -> None:
        pads = np.ascontiguousarray(pad_left, dtype=np.int32)
        if pads.shape != (r,):
            raise ValueError("one pad per row")
        self._check(self._lib.pal_align_rows_dev(self._h, C.c_void_p(d_rows), int(r), int(n), pads.ctypes.data, int(lout), C.c_void_p(d_out)))

    def filtfilt_dev(self, b, a, zi, d_rows: int, r: int, n: int, d_out: int) -> None:
        b, a, zi = f64(b), f64(a), f64(zi)
        self._check(self._lib.pal_filtfilt_dev(self._h, b.ctypes.data, b.shape[0], a.ctypes.data, a.shape[0], zi.ctypes.data,
                                               C.c_void_p(d_rows), int(r), int(n), C.c_void_p(d_out)))

    def filtfilt_ragged_dev(self, b, a, zi, d_in: int, d_out: int, in_off, out_off, lengths) -> None:
        """Rows of different lengths in one launch: row r = d_in[in_off[r] : + lengths[r]] -> d_out[out_off[r] : ...] (offsets in doubles)."""
        b, a, zi = f64(b), f64(a), f64(zi)
        io = np.ascontiguousarray(in_off, dtype=np.int64)
        oo = np.ascontiguousarray(out_off, dtype=np.int64)
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        if not (io.shape == oo.shape == ln.shape) or io.ndim != 1:
            raise ValueError("one offset pair and one length per row")
        self._check(self._lib.pal_filtfilt_ragged_dev(self._h, b.ctypes.data, b.shape[0], a.ctypes.data, a.shape[0], zi.ctypes.data,
                                                      C.c_void_p(d_in), C.c_void_p(d_out), io.shape[0], io.ctypes.data, oo.ctypes.data,
                                                      ln.ctypes.data))

    def wiener3_dev(self, d_rows: int, r: int, n: int, d_out: int) -> None:
        self._check(self._lib.pal_wiener3_dev(self._h, C.c_void_p(d_rows), int(r), int(n), C.c_void_p(d_out)))

    # ---- recorded audio: resample, normalise, cut frames (stream.recorded_tdoa_stream) -------------
    def resample_set_filter(self, win, num_table: int) -> None:
        """The right wing of the interpolation filter and its table entries per zero crossing (once per engine)."""
        w = f64(win)
        if w.ndim != 1:
            raise ValueError("the filter wing is one-dimensional")
        self._check(self._lib.pal_resample_set_filter(self._h, w.ctypes.data, w.shape[0], int(num_table)))
        self._resample_filter = True

    def _resample_length(self, n: int, original_fs, target_fs) -> int:
        """Output length and errors of signal_processing.resample_kaiser_best; hands the engine the filter on first use."""
        ratio = float(target_fs) / float(original_fs)
        if ratio <= 0:
            raise ValueError("Invalid sample rates")
        n_out = int(n * ratio)
        if n_out < 1:
            raise ValueError(f"Input signal length={n} is too small to resample from {original_fs}->{target_fs}")
        if not getattr(self, "_resample_filter", False):
            from .signal_processing import _kaiser_best_filter  # noqa: PLC0415 - signal_processing imports this module
            self.resample_set_filter(*_kaiser_best_filter())
        return n_out

    def resample(self, rows, original_fs, target_fs) -> np.ndarray:
        """signal_processing.resample_kaiser_best along the last axis of rows[R][N] (or [N]) on the device, bit for bit."""
        x = f64(rows)
        if x.ndim == 0:
            raise ValueError("rows must have a sample axis")
        lead, n = x.shape[:-1], x.shape[-1]
        n_out = self._resample_length(n, original_fs, target_fs)
        x2 = x.reshape(-1, n)
        out = np.empty((x2.shape[0], n_out))
        if x2.shape[0] == 0:
            return out.reshape(lead + (n_out,))
        got = C.c_int()
        self._check(self._lib.pal_resample(self._h, x2.ctypes.data, x2.shape[0], n, float(original_fs), float(target_fs), out.ctypes.data,
                                           n_out, C.byref(got)))
        assert got.value == n_out
        return out.reshape(lead + (n_out,))

    def resample_dev(self, d_rows: int, r: int, n: int, original_fs, target_fs, d_out: int, n_out_capacity: int) -> int:
        """Asynchronous: d_rows[r][n] -> d_out[r][n_out] in HBM; returns n_out = int(n * target_fs / original_fs)."""
        n_out = self._resample_length(int(n), original_fs, target_fs)
        got = C.c_int()
        self._check(self._lib.pal_resample_dev(self._h, C.c_void_p(d_rows), int(r), int(n), float(original_fs), float(target_fs),
                                               C.c_void_p(d_out), int(n_out_capacity), C.byref(got)))
        assert got.value == n_out
        return n_out

    def normalize_compress_dev(self, d_rows: int, r: int, n: int, d_out: int, normalize_only=False, threshold=0.8, epsilon=1e-8) -> None:
        """Asynchronous: normalize_compress on d_rows[r][n] -> d_out[r][n] in HBM (d_out may be d_rows)."""
        self._check(self._lib.pal_normalize_compress_dev(self._h, C.c_void_p(d_rows), int(r), int(n), int(normalize_only), float(threshold),
                                                         float(epsilon), C.c_void_p(d_out)))

    def frame_rows_dev(self, d_rows: int, m: int, t: int, frame_len: int, hop: int, first_frame: int, frames: int, d_out: int) -> None:
        """Asynchronous: d_out[f][m][i] = d_rows[m][(first_frame + f) * hop + i]; a frame past sample t raises ValueError."""
        self._check(self._lib.pal_frame_rows_dev(self._h, C.c_void_p(d_rows), int(m), int(t), int(frame_len), int(hop), int(first_frame),
                                                 int(frames), C.c_void_p(d_out)))

    # ---- multi-GPU ---------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = _ffi.load().pal_comm_unique_id(buf)
        if rc != 0:
            raise PalError(rc, "ncclGetUniqueId failed (librccl not loadable?)")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, unique_id: bytes) -> None:
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self._lib.pal_comm_init(self._h, int(nranks), int(rank), buf))

    def all_gather_dev(self, d_send: int, d_recv: int, nbytes_per_rank: int) -> None:
        self._check(self._lib.pal_comm_all_gather(self._h, C.c_void_p(d_send), C.c_void_p(d_recv), int(nbytes_per_rank)))

    def comm_destroy(self) -> None:
        self._check(self._lib.pal_comm_destroy(self._h))

    # ---- measurement ---------------------------------------------------------------------
    def profile_begin(self, every: int = 1) -> None:
        """Bracket the engine's launches with HIP events (every `every`-th launch group of the pair pipeline)."""
        self._check(self._lib.pal_profile_sampling(self._h, int(every)))
        self._check(self._lib.pal_profile_begin(self._h))

    def profile_end(self) -> None:
        self._check(self._lib.pal_profile_end(self._h))

    def profile_get(self, name: str) -> Tuple[float, int]:
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._lib.pal_profile_get(self._h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


    def profile_entries(self) -> dict:
        """{kernel instance name: (total ms, launches)} accumulated since profile_begin()."""
        out = {}
        idx = 0
        while True:
            name = C.create_string_buffer(96)
            ms, cnt = C.c_double(), C.c_int64()
            if self._lib.pal_profile_entry(self._h, idx, name, 96, C.byref(ms), C.byref(cnt)) != 0:
                return out
            out[name.value.decode()] = (ms.value, cnt.value)
            idx += 1


def image_sources(source, planes, material_id, absorption, freq_coeff, max_order, frequency, mics, threshold=0.01,
                  round_decimals=6, cap=4096):
    """Host C++ breadth-first image-source search (utils.py:67-106) -> (images[count][3], material index[count])."""
    lib = _ffi.load()
    src = f64(source, (3,))
    pl = f64(planes).reshape(-1, 4) if len(planes) else np.zeros((0, 4))
    mid = np.ascontiguousarray(material_id, dtype=np.int32)
    ab, fc = f64(absorption), f64(freq_coeff)
    mic = f64(mics).reshape(-1, 3)
    img = np.zeros((cap, 3))
    mat = np.zeros(cap, dtype=np.int32)
    cnt = C.c_int()
    rc = lib.pal_image_sources(src.ctypes.data, pl.ctypes.data, mid.ctypes.data, pl.shape[0], ab.ctypes.data, fc.ctypes.data,
                               ab.shape[0], int(max_order), float(frequency), mic.ctypes.data, mic.shape[0],
                               float(threshold), int(round_decimals), img.ctypes.data, mat.ctypes.data, cap, C.byref(cnt))
    if rc == _ffi.ERR_INVALID:
        raise ValueError("invalid plane (a^2 + b^2 + c^2 == 0) or material index")
    if rc == _ffi.ERR_MATERIAL:
        raise KeyError(cnt.value)                              # plane index whose material is undefined
    if rc != 0:
        raise PalError(rc, f"image source capacity {cap} exceeded ({cnt.value} found)")
    return img[: cnt.value].copy(), mat[: cnt.value].copy()


_default: Optional[Engine] = None


def default_engine() -> Engine:
    """Process-wide engine used by the drop-in modules (device from PAL_DEVICE, default 0)."""
    global _default
    if _default is None:
        _default = Engine()
    return _default
