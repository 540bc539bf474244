"""TDOA table -> source position: the batched device solve (csrc/solve.hip, pal_solve_positions*) restated in NumPy.

The reference's tail (main.py:233-298) clusters per-pair points with scikit-learn for its start points and runs SciPy's
bounded trust-region least squares from each.  The device path keeps the reference's residuals, weights and box and
replaces the rest by something a workgroup can iterate on its own: a fixed list of start points and a bounded
Levenberg-Marquardt iteration on sixteen fp64 sums over the frame's pairs.  This module is the specification - the kernels
follow it step by step (the arithmetic lives in csrc/solve_math.h) and differ from it only in the order of the sums over
the pairs.

Per frame, from the 48-byte record table (``_ffi.RECORD``, row-major i<j) and the frame's length L:

- ``td[p] = (k_sel[p] - (L - 1)) / fs``, minus ``calib[j] - calib[i]`` when calibration delays are given (main.py:209-212);
- weights ``w``: ones, ``snr / mean(snr)`` exactly as ``utils.compute_weights`` (NumPy's pairwise mean included), or a
  caller's array.  A frame whose weights are not all finite is not solved (``ST_BAD_WEIGHTS``);
- box: ``utils.dynamic_bounds_extended``: microphone extents -/+ (buffer + max(1, 75th percentile of c |td|));
- residuals ``r_p = (d_j - d_i) w_p - b_p`` with ``b_p = (c td_p) w_p``, cost = sum(r^2) / 2 (utils.py:384-405);
- starts: 0 = the mean microphone position, 1 .. g^3 = the cell centres of a g x g x g grid over the box (x slowest),
  then the caller's extra starts clipped to the box;
- iteration per start (``lm_solve``): Jacobian rows ``w_p (u_j - u_i)`` and sixteen sums over the pairs: JtJ (6), Jtr (3), rtr (1) and
  the second-order part of the Hessian, ``sum r_p w_p (H_j - H_i)`` with ``H_m = (I - u_m u_m^t) / d_m`` (6).  A coordinate that sits on a
  face of the box with the cost's gradient pointing outward is held.  The step solves ``(H + lam diag(JtJ)) delta = -Jtr`` on the free
  block, with H the full Hessian where that matrix is positive definite and JtJ otherwise, and is clipped to the box.  A trial point is
  accepted when it lowers rtr (``lam`` then follows Nielsen's gain-ratio rule, not below ``LAM_MIN``) and rejected otherwise
  (``lam *= nu``, ``nu *= 2``).  Every trial point counts as one iteration.

Stop rules (``STOP_*``), every one of them a converged end except the cap:

- gradient: for every free coordinate ``|Jtr_k| <= GTOL sqrt(JtJ_kk rtr)`` - the cosine between the residual vector and that column of
  the Jacobian, scale-free; 1e-8 is where an accept-on-decrease test stops resolving rtr in float64;
- step: a trial step with ``max |s_k| <= XTOL (XTOL + max |x_k|)``;
- decrease: an accepted step that lowers rtr by no more than ``FTOL rtr`` while ``lam <= 1`` (a step shortened by heavy damping says
  nothing about convergence);
- damping: ``lam > LAM_MAX`` - no representable step lowers the cost;
- cap: ``max_iter`` trial points (``ST_HIT_CAP``).

The tables of the reference's fixtures are large-residual problems (the C3 table's optimum has an rms residual of 5 m, the five-microphone
table's optimum sits 13 um from a microphone, where the cost has a cone).  Gauss-Newton steps alone contract slowly there: with the ten
sums JtJ, Jtr, rtr the C3 table ended in a worse minimum than the reference's and most starts of the five-microphone table ran into a
cap of 200; with the second-order sums the winners of the fixtures end inside a stop rule after 6 to 98 trial points.

Winner of a frame: the lowest cost among the starts that ended inside a stop rule, exact ties to the lowest start index.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

ST_CONVERGED, ST_HIT_CAP, ST_BAD_WEIGHTS, ST_ON_FACE = 1, 2, 4, 8      # PAL_SOLVE_* status bits
STOP_NONE, STOP_GRADIENT, STOP_STEP, STOP_DECREASE, STOP_DAMPING, STOP_CAP = 0, 1, 2, 3, 4, 5
WEIGHTS = {"ones": 0, "snr": 1, "array": 2}                             # PAL_SOLVE_W_*
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2, "cauchy": 3}           # PAL_SOLVE_LOSS_*

GTOL = 1e-8
XTOL = 1e-13
FTOL = 1e-13
LAM0 = 1e-3
LAM_MIN = 1e-9
LAM_MAX = 1e12
MAX_ITER = 200
GRID = 4
MAX_GRID = 16
MAX_MICS = 256

# one row of the result (pal_position_record, 96 bytes)
POSITION = np.dtype([("position", "<f8", (3,)), ("cost", "<f8"), ("lower", "<f8", (3,)), ("upper", "<f8", (3,)),
                     ("start", "<i4"), ("iterations", "<i4"), ("converged_starts", "<i4"), ("status", "<i4")])
assert POSITION.itemsize == 96


def pair_indices(mics: int):
    i, j = np.triu_indices(int(mics), k=1)
    return i.astype(np.int64), j.astype(np.int64)


def time_delays(k_sel, length: int, fs: float, calib=None, mics: Optional[int] = None) -> np.ndarray:
    k = np.asarray(k_sel, dtype=np.int64)
    td = (k - (int(length) - 1)) / float(fs)
    if calib is not None:
        cal = np.asarray(calib, dtype=np.float64)
        i, j = pair_indices(cal.shape[0] if mics is None else mics)
        td = td - (cal[j] - cal[i])
    return td


def snr_weights(snr) -> np.ndarray:
    """utils.compute_weights on an SNR column."""
    w = np.ascontiguousarray(snr, dtype=np.float64)
    mean = np.mean(w)
    return w / mean if mean != 0 else w


def percentile75(values) -> float:
    """np.percentile(values, 75) by rank selection: virtual index 0.75 (P - 1), NumPy's linear interpolation."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    h = 0.75 * (v.shape[0] - 1)
    lo = int(np.floor(h))
    t = h - lo
    a, b = v[lo], v[min(lo + 1, v.shape[0] - 1)]
    d = b - a
    out = a + d * t if t < 0.5 else b - d * (1 - t)
    return float(a if d == 0 else out)


def box(mics, td, c: float, buffer: float = 5.0):
    mics = np.asarray(mics, dtype=np.float64)
    extra = max(percentile75(c * np.abs(td)), 1.0)
    return mics.min(axis=0) - (buffer + extra), mics.max(axis=0) + (buffer + extra)


def start_points(mics, lower, upper, grid: int = GRID, extra=None) -> np.ndarray:
    mics = np.asarray(mics, dtype=np.float64)
    centre = np.zeros(3)
    for row in mics:                                   # row by row, like np.mean(mics, axis=0)
        centre = centre + row
    out = [centre / mics.shape[0]]
    g = int(grid)
    h = (upper - lower) / g if g else None
    for ix in range(g):
        for iy in range(g):
            for iz in range(g):
                out.append(lower + (np.array([ix, iy, iz]) + 0.5) * h)
    if extra is not None:
        for e in np.asarray(extra, dtype=np.float64).reshape(-1, 3):
            out.append(np.minimum(np.maximum(e, lower), upper))
    return np.array(out)


def sums(x, mics, pi, pj, b, w):
    """The sixteen sums at x: JtJ and the second-order part of the Hessian, sum r_p w_p (H_j - H_i) with
    H_m = (I - u_m u_m^t) / d_m, both as (xx, xy, xz, yy, yz, zz); Jtr; rtr."""
    diff = x - mics
    d = np.sqrt(np.sum(diff * diff, axis=1))
    inv = 1.0 / np.where(d > 0, d, np.inf)
    u = diff * inv[:, None]
    r = (d[pj] - d[pi]) * w - b
    jac = (u[pj] - u[pi]) * w[:, None]
    rw = r * w
    ia, ib = [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]
    h = (np.eye(3)[ia, ib][None, :] - u[:, ia] * u[:, ib]) * inv[:, None]          # [M][6]
    a6 = np.sum(jac[:, ia] * jac[:, ib], axis=0)
    s6 = np.sum(rw[:, None] * (h[pj] - h[pi]), axis=0)
    return a6, s6, jac.T @ r, float(r @ r)


def check_loss(loss, f_scale):
    """-> (PAL_SOLVE_LOSS_* code, f_scale as a float); ValueError on an unknown loss or an f_scale that is not finite and positive."""
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError("loss: one of " + ", ".join(repr(k) for k in LOSSES))
    try:
        scale = float(f_scale)
    except (TypeError, ValueError):
        raise ValueError("f_scale must be a number") from None
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("f_scale must be finite and positive")
    return LOSSES[loss], scale


def loss_terms(loss: str, z):
    """rho(z), rho'(z) and rho'(z) + 2 z rho''(z) clamped at zero (Triggs' correction as SciPy applies it), written without
    cancellation at small z like solve_math.h."""
    z = np.asarray(z, dtype=np.float64)
    if loss == "soft_l1":
        t = np.sqrt(1.0 + z)
        a = 1.0 / t
        return 2.0 * z / (t + 1.0), a, a / (1.0 + z)
    if loss == "huber":
        inner = z <= 1.0
        t = np.sqrt(np.where(inner, 1.0, z))
        return np.where(inner, z, 2.0 * t - 1.0), np.where(inner, 1.0, 1.0 / t), np.where(inner, 1.0, 0.0)
    if loss == "cauchy":
        a = 1.0 / (1.0 + z)
        return np.log1p(z), a, np.maximum((1.0 - z) * a * a, 0.0)
    raise ValueError("loss_terms: a robust loss")


def sums_loss(x, mics, pi, pj, b, w, loss: str, f_scale: float):
    """The nineteen sums of a robust loss at x, z_p = r_p^2 / C^2, a_p = rho'(z_p), c_p = max(rho' + 2 z rho'', 0):
    sum c_p j j^t, sum a_p r_p w_p (H_j - H_i), the gradient sum a_p r_p j_p, C^2 sum rho(z_p) in place of rtr, and
    sum a_p j_k^2 (the diagonal of Marquardt's scaling and of the gradient stop rule)."""
    diff = x - mics
    d = np.sqrt(np.sum(diff * diff, axis=1))
    inv = 1.0 / np.where(d > 0, d, np.inf)
    u = diff * inv[:, None]
    r = (d[pj] - d[pi]) * w - b
    jac = (u[pj] - u[pi]) * w[:, None]
    c2 = f_scale * f_scale
    rho, a, c = loss_terms(loss, (r * r) * (1.0 / c2))
    ar = a * r
    ia, ib = [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]
    h = (np.eye(3)[ia, ib][None, :] - u[:, ia] * u[:, ib]) * inv[:, None]          # [M][6]
    a6 = np.sum(c[:, None] * (jac[:, ia] * jac[:, ib]), axis=0)
    s6 = np.sum((ar * w)[:, None] * (h[pj] - h[pi]), axis=0)
    return a6, s6, jac.T @ ar, float(c2 * np.sum(rho)), np.sum(a[:, None] * (jac * jac), axis=0)


def pair_weights(x, mics, pi, pj, b, w, loss: str, f_scale: float) -> np.ndarray:
    """rho'(z_p) at x: how much of each pair's residual the fit kept (ones for the linear loss)."""
    if loss == "linear":
        return np.ones(np.asarray(b).shape[0])
    d = np.sqrt(np.sum((x - np.asarray(mics, dtype=np.float64)) ** 2, axis=1))
    r = (d[pj] - d[pi]) * w - b
    return loss_terms(loss, (r * r) * (1.0 / (f_scale * f_scale)))[1]


def held_coordinates(x, g, lower, upper) -> np.ndarray:
    return ((x <= lower) & (g > 0)) | ((x >= upper) & (g < 0))


def damped_step(h6, d3, g, lam: float, held):
    """Solve (H + lam diag(d3)) delta = -g on the free coordinates (held ones: delta = 0) by an LDLt factorisation without
    pivoting; (ok, delta) - not ok when a pivot is not positive."""
    xx, xy, xz, yy, yz, zz = (float(v) for v in h6)
    m = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    rhs = -np.asarray(g, dtype=np.float64)
    for k in range(3):
        m[k, k] = m[k, k] + lam * d3[k]
    for k in range(3):
        if held[k]:
            m[k, :] = 0.0
            m[:, k] = 0.0
            m[k, k] = 1.0
            rhs[k] = 0.0
    d0 = m[0, 0]
    if not d0 > 0:
        return False, np.zeros(3)
    l10, l20 = m[1, 0] / d0, m[2, 0] / d0
    d1 = m[1, 1] - l10 * m[1, 0]
    if not d1 > 0:
        return False, np.zeros(3)
    l21 = (m[2, 1] - l20 * m[1, 0]) / d1
    d2 = m[2, 2] - l20 * m[2, 0] - l21 * (l21 * d1)
    if not d2 > 0:
        return False, np.zeros(3)
    y0 = rhs[0]
    y1 = rhs[1] - l10 * y0
    y2 = rhs[2] - l20 * y0 - l21 * y1
    z2 = y2 / d2
    z1 = y1 / d1 - l21 * z2
    z0 = y0 / d0 - l10 * z1 - l20 * z2
    return True, np.array([z0, z1, z2])


def quad_form(h6, s) -> float:
    return float(h6[0] * s[0] * s[0] + h6[3] * s[1] * s[1] + h6[5] * s[2] * s[2]
                 + 2.0 * (h6[1] * s[0] * s[1] + h6[2] * s[0] * s[2] + h6[4] * s[1] * s[2]))


def lm_solve(x0, lower, upper, mics, pi, pj, b, w, max_iter: int = MAX_ITER, loss: str = "linear", f_scale: float = 1.0):
    """-> (x, cost, iterations, stop rule)."""
    if loss != "linear":
        return lm_solve_loss(x0, lower, upper, mics, pi, pj, b, w, max_iter, loss, f_scale)
    mics = np.asarray(mics, dtype=np.float64)
    x = np.minimum(np.maximum(np.asarray(x0, dtype=np.float64), lower), upper)
    a6, s6, g, f = sums(x, mics, pi, pj, b, w)
    lam, nu, it = LAM0, 2.0, 0
    while True:
        held = held_coordinates(x, g, lower, upper)
        diag = np.array([a6[0], a6[3], a6[5]])
        if np.all(held | (np.abs(g) <= GTOL * np.sqrt(diag * f))):
            stop = STOP_GRADIENT
            break
        if it >= max_iter:
            stop = STOP_CAP
            break
        it += 1
        h6 = a6 + s6                                   # the full Hessian where its damped free block is positive definite,
        ok, delta = damped_step(h6, diag, g, lam, held)
        if not ok:                                     # the Gauss-Newton matrix otherwise
            h6 = a6
            ok, delta = damped_step(h6, diag, g, lam, held)
        if ok:
            xn = np.minimum(np.maximum(x + delta, lower), upper)
            s = xn - x
            if np.max(np.abs(s)) <= XTOL * (XTOL + np.max(np.abs(x))):
                stop = STOP_STEP
                break
            an, sn, gn, fn = sums(xn, mics, pi, pj, b, w)
        if ok and fn < f:
            pred = -(2.0 * float(g @ s) + quad_form(h6, s))
            rho = (f - fn) / pred if pred > 0 else 1.0
            small = (f - fn) <= FTOL * f and lam <= 1.0
            x, a6, s6, g, f = xn, an, sn, gn, fn
            t = 2.0 * rho - 1.0
            lam = max(lam * max(1.0 / 3.0, 1.0 - t * t * t), LAM_MIN)
            nu = 2.0
            if small:
                stop = STOP_DECREASE
                break
        else:
            lam = lam * nu
            nu = 2.0 * nu
            if lam > LAM_MAX:
                stop = STOP_DAMPING
                break
    return x, 0.5 * f, it, stop


def lm_solve_loss(x0, lower, upper, mics, pi, pj, b, w, max_iter: int, loss: str, f_scale: float):
    """lm_solve on the robust cost F = sum C^2 rho(r^2 / C^2) / 2: f is 2 F, g its gradient, the matrix sum c_p j j^t (plus the
    second-order part where the damped free block stays positive definite), Marquardt's diagonal sum a_p j_k^2."""
    mics = np.asarray(mics, dtype=np.float64)
    x = np.minimum(np.maximum(np.asarray(x0, dtype=np.float64), lower), upper)
    a6, s6, g, f, diag = sums_loss(x, mics, pi, pj, b, w, loss, f_scale)
    lam, nu, it = LAM0, 2.0, 0
    while True:
        held = held_coordinates(x, g, lower, upper)
        if np.all(held | (np.abs(g) <= GTOL * np.sqrt(diag * f))):
            stop = STOP_GRADIENT
            break
        if it >= max_iter:
            stop = STOP_CAP
            break
        it += 1
        h6 = a6 + s6
        ok, delta = damped_step(h6, diag, g, lam, held)
        if not ok:
            h6 = a6
            ok, delta = damped_step(h6, diag, g, lam, held)
        if ok:
            xn = np.minimum(np.maximum(x + delta, lower), upper)
            s = xn - x
            if np.max(np.abs(s)) <= XTOL * (XTOL + np.max(np.abs(x))):
                stop = STOP_STEP
                break
            an, sn, gn, fn, dn = sums_loss(xn, mics, pi, pj, b, w, loss, f_scale)
        if ok and fn < f:
            pred = -(2.0 * float(g @ s) + quad_form(h6, s))
            rho = (f - fn) / pred if pred > 0 else 1.0
            small = (f - fn) <= FTOL * f and lam <= 1.0
            x, a6, s6, g, f, diag = xn, an, sn, gn, fn, dn
            t = 2.0 * rho - 1.0
            lam = max(lam * max(1.0 / 3.0, 1.0 - t * t * t), LAM_MIN)
            nu = 2.0
            if small:
                stop = STOP_DECREASE
                break
        else:
            lam = lam * nu
            nu = 2.0 * nu
            if lam > LAM_MAX:
                stop = STOP_DAMPING
                break
    return x, 0.5 * f, it, stop


def solve_frame(k_sel, length: int, mics, fs: float, c: float, calib=None, weights="ones", snr=None, buffer: float = 5.0,
                grid: int = GRID, max_iter: int = MAX_ITER, extra_starts=None, return_starts: bool = False,
                loss: str = "linear", f_scale: float = 1.0):
    """One frame -> a POSITION record (``weights``: 'ones', 'snr' (needs ``snr``), or an array of P weights; ``loss``: one of
    LOSSES with scale ``f_scale``, in metres of weighted residual)."""
    _, f_scale = check_loss(loss, f_scale)
    mics = np.asarray(mics, dtype=np.float64)
    m = mics.shape[0]
    pi, pj = pair_indices(m)
    td = time_delays(k_sel, length, fs, calib, m)
    if td.shape[0] != pi.shape[0]:
        raise ValueError("the table must have M (M - 1) / 2 rows")
    if isinstance(weights, str):
        if weights not in ("ones", "snr"):
            raise ValueError("weights: 'ones', 'snr' or an array")
        w = np.ones(td.shape[0]) if weights == "ones" else snr_weights(snr)
    else:
        w = np.ascontiguousarray(weights, dtype=np.float64)
    rec = np.zeros((), dtype=POSITION)
    lower, upper = box(mics, td, c, buffer)
    rec["lower"], rec["upper"] = lower, upper
    if not np.all(np.isfinite(w)):
        rec["position"] = np.nan
        rec["cost"] = np.nan
        rec["start"] = -1
        rec["status"] = ST_BAD_WEIGHTS
        return (rec, None, None) if return_starts else rec
    b = (c * td) * w
    starts = start_points(mics, lower, upper, grid, extra_starts)
    if loss == "linear":
        results = [lm_solve(s, lower, upper, mics, pi, pj, b, w, max_iter) for s in starts]
    else:
        results = [lm_solve_loss(s, lower, upper, mics, pi, pj, b, w, max_iter, loss, f_scale) for s in starts]
    best, best_capped, nconv = -1, -1, 0
    for k, (_, cost, _, stop) in enumerate(results):
        if stop != STOP_CAP:
            nconv += 1
            if best < 0 or cost < results[best][1]:
                best = k
        elif best_capped < 0 or cost < results[best_capped][1]:
            best_capped = k
    win = best if best >= 0 else best_capped
    x, cost, it, stop = results[win]
    rec["position"], rec["cost"], rec["start"], rec["iterations"], rec["converged_starts"] = x, cost, win, it, nconv
    status = ST_CONVERGED if best >= 0 else ST_HIT_CAP
    if np.any((x <= lower) | (x >= upper)):
        status |= ST_ON_FACE
    rec["status"] = status
    return (rec, starts, results) if return_starts else rec
