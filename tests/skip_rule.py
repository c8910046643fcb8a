"""The skip-distance rule and the MUF bisection of DESIGN.md section 4.10 in NumPy, driven by callables: a helper of
tests/test_skip_rule_host.py, tests/test_gpu_skip.py and tools/gen_golden_skip.py, not a test.

Every operation below is one float64 operation of the kernels (prhf_skip.inc), in the same order, so that a driver
whose D(e) returns the tracer's own bits reproduces the kernel's elevation, status, n_evals and bracket bit for bit."""

import math

import numpy as np

GOLD = 0.3819660112501051
INF = float("inf")


def scan_node(d):
    """(i*, edge) of a scan's ground ranges d (E,): the first index that attains the minimum over the finite d, or
    -1 when none is finite; edge: i* is 0, E - 1, or has a neighbour that is not finite."""
    d = np.asarray(d, dtype=np.float64)
    ok = np.isfinite(d)
    if not ok.any():
        return -1, False
    i = int(np.argmin(np.where(ok, d, np.inf)))                     # (np.argmin returns the first index of the minimum)
    edge = i == 0 or i == d.size - 1 or not ok[i - 1] or not ok[i + 1]
    return i, edge


def skip_search(scan, d, ray, elev_tol_deg=1e-6, max_iter=64):
    """The rule on the scan grid `scan` (E,) with ground ranges `d` (E,); ray(e) -> ground range of the group's ray at
    elevation e (NaN: it does not turn).  Returns a dict: status, scan_index, elevation_deg (b), skip_km (D at b),
    bracket_deg, n_evals, and `triple` (a, b, c) at the end."""
    scan = np.asarray(scan, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    i, edge = scan_node(d)
    nan = float("nan")
    if i < 0:
        return dict(status=-1, scan_index=-1, elevation_deg=nan, skip_km=nan, bracket_deg=nan, n_evals=0, triple=(nan,) * 3)
    if edge:
        return dict(status=1, scan_index=i, elevation_deg=float(scan[i]), skip_km=float(d[i]), bracket_deg=nan, n_evals=0,
                    triple=(nan, float(scan[i]), nan))
    a, b, c, db = float(scan[i - 1]), float(scan[i]), float(scan[i + 1]), float(d[i])
    tol, n, status = float(elev_tol_deg), 0, 3
    for _ in range(max_iter + 1):
        if c - a <= tol:
            status = 0
            break
        right = (c - b) >= (b - a)
        x = b + GOLD * (c - b) if right else b - GOLD * (b - a)
        if not (a < x < c) or x == b:
            status = 0
            break
        if n >= max_iter:
            status = 3
            break
        dx = float(ray(x))
        n += 1
        if not math.isfinite(dx):
            status = 2
            break
        if dx < db:
            if right:
                a = b
            else:
                c = b
            b, db = x, dx
        elif right:
            c = x
        else:
            a = x
    return dict(status=status, scan_index=i, elevation_deg=b, skip_km=db, bracket_deg=c - a, n_evals=n, triple=(a, b, c))


def muf_search(s, t, f_lo, f_hi, n_bisect=40):
    """The bisection on a skip-distance function s(f) (+inf where no ray lands) for the target t.  Returns a dict:
    status, muf_hz, f_above_hz, and `trips`: the list of (m, s(m), lo, hi before the trip) of the trips that moved an
    end."""
    nan = float("nan")
    if t != t:
        return dict(status=-1, muf_hz=nan, f_above_hz=nan, trips=[])
    if s(f_lo) > t:
        return dict(status=2, muf_hz=nan, f_above_hz=nan, trips=[])
    if s(f_hi) <= t:
        return dict(status=1, muf_hz=float(f_hi), f_above_hz=nan, trips=[])
    lo, hi, trips = float(f_lo), float(f_hi), []
    for _ in range(n_bisect):
        m = lo + 0.5 * (hi - lo)
        if not lo < m < hi:
            continue
        sm = s(m)
        trips.append((m, sm, lo, hi))
        if sm <= t:
            lo = m
        else:
            hi = m
    return dict(status=0, muf_hz=lo, f_above_hz=hi, trips=trips)


def slope_sign_changes(d):
    """How often the slope of the samples d changes its sign (flat steps skipped): 1 for a unimodal dip."""
    s = np.sign(np.diff(np.asarray(d, dtype=np.float64)))
    s = s[s != 0]
    return int(np.count_nonzero(s[1:] != s[:-1]))


def largest_slope(e, d):
    """The largest |dD / de| between neighbouring samples."""
    return float(np.max(np.abs(np.diff(d) / np.diff(e))))
