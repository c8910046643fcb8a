"""The bracket and refine rules of gradient homing restated in plain Python: float64 operations
in the order include/prhf.h writes them out for prhf_gradient_home_f64, so that driving any tracer through `refine`
reproduces the elevations the kernel tries, bit for bit.  Used by tools/gen_golden_gradient_homing.py (driving the
reference's tracer) and by the tests (driving a synthetic D(e), or the GPU tracer one ray per call)."""

import math


def brackets(d, t):
    """Intervals of the scan `d` (ground ranges, NaN where the ray does not land) that bracket the target `t`, in
    ascending order; len(d) - 1 stands for the bracket of no width at the last node."""
    n = len(d)
    if t != t:
        return []
    found = []
    for i in range(n):
        d0 = float(d[i])
        if i == n - 1:
            if d0 == t:
                found.append(i)
            continue
        d1 = float(d[i + 1])
        f0, f1 = d0 - t, d1 - t
        if math.isfinite(d0) and math.isfinite(d1) and ((f0 < 0.0 and f1 > 0.0) or (f0 > 0.0 and f1 < 0.0) or d0 == t):
            found.append(i)
    return found


def refine(ray, scan, d, i, t, tol, max_iter):
    """Refine bracket `i` of the scan (`scan` elevations, `d` ground ranges) towards the target `t`.  `ray(e)` is the
    ground range of the ray at elevation e, NaN when it does not land.  Returns a dict: status (0 converged, 1 the
    midpoint left the bracket or max_iter is spent, 2 a ray inside does not land), elevation and miss of the best ray,
    whether that ray is a scan node, the elevations tried and how often a step at least halved the bracket."""
    t = float(t)
    lo, f_lo = float(scan[i]), float(d[i]) - t
    wide = i + 1 < len(scan)
    hi = float(scan[i + 1]) if wide else lo
    f_hi = float(d[i + 1]) - t if wide else f_lo
    best_e = hi if abs(f_hi) < abs(f_lo) else lo
    best_miss = min(abs(f_lo), abs(f_hi))
    best_is_node = True
    status = 0 if best_miss <= tol else 1
    tried, halved = [], 0
    if status != 0:
        g_lo, g_hi = f_lo, f_hi
        last_side, bisect = 0, False
        for _ in range(max_iter):
            mid = lo + 0.5 * (hi - lo)
            if not (lo < mid < hi):
                break
            x = mid
            if not bisect:
                xs = lo - g_lo * ((hi - lo) / (g_hi - g_lo))
                if lo < xs < hi:
                    x = xs
            dx = float(ray(x))
            tried.append(x)
            if not math.isfinite(dx):
                status = 2
                break
            f = dx - t
            miss = abs(f)
            if miss < best_miss:
                best_miss, best_e, best_is_node = miss, x, False
            if miss <= tol:
                status = 0
                break
            width = hi - lo
            if (f < 0.0) == (f_lo < 0.0):
                lo, f_lo, g_lo = x, f, f
                if last_side == -1:
                    g_hi = 0.5 * g_hi
                last_side = -1
            else:
                hi, g_hi = x, f
                if last_side == 1:
                    g_lo = 0.5 * g_lo
                last_side = 1
            bisect = (hi - lo) > 0.5 * width
            if not bisect:
                halved += 1
    return {"status": status, "elevation_deg": best_e, "miss_km": best_miss, "is_node": best_is_node, "tried": tried,
            "halved": halved}
