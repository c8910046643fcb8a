"""The Levenberg-Marquardt rule of DESIGN.md section 4.16 in NumPy, driven by a callable: a helper of
tests/test_lm_fit_host.py, tests/test_gpu_lm_fit.py, tests/test_gpu_lm_fit_edges.py and tools/bench_lm_fit.py, not a test.

Every operation below is one float64 operation of pyrayhf_amd/csrc/prhf_lm_step.h, in the same order (no fused
multiply-add; the sums over the frequencies in the wavefront's order: 64 lane sums over f = l, l + 64, ..., then the
pairwise tree of ``wave_order_sum``), so that a driver whose ``evaluate(c)`` returns the device's own ``vh`` and ``dvh``
bits reproduces lm_step_kernel's state bit for bit, and tests/devtools/lm_step_host.cpp on the same linear model does too."""

import math

import numpy as np

RUNNING, CONVERGED_F, CONVERGED_X, SINGULAR, NO_DATA, NO_COST = range(6)
RETRIES = 8
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
TINY = 1e-30
DEFAULTS = dict(max_iter=20, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, step_max=1.0, ftol=1e-10, xtol=1e-10)
NAN = float("nan")
_LANES = np.arange(64)


def clamp(lam):
    return LAMBDA_MIN if lam < LAMBDA_MIN else (LAMBDA_MAX if lam > LAMBDA_MAX else lam)


def wave_order_sum(lanes):
    """The sum of 64 lane values (..., 64) in wave_sum's order: v[l] + v[l ^ 32], then ^ 16, 8, 4, 2, 1."""
    v = np.array(lanes, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ off]
    return v[..., 0]


def lane_sums(terms):
    """Per-lane sums (..., 64) of terms (n, ...) taken in order: lane l adds the terms l, l + 64, ..."""
    terms = np.asarray(terms, dtype=np.float64)
    out = np.zeros((64,) + terms.shape[1:])
    for j in range(terms.shape[0]):
        out[j % 64] = out[j % 64] + terms[j]
    return np.moveaxis(out, 0, -1)


def eval_sums(vh_obs, vh_model, dvh):
    """lm_step_kernel's sums for one ionogram: ``(A (T, T), g (T,), cost, n_kept)`` of the data alone.  Frequencies
    stay on their own lane (f mod 64) whether kept or not."""
    vh_obs, vh_model = np.asarray(vh_obs, dtype=np.float64), np.asarray(vh_model, dtype=np.float64)
    dvh = np.asarray(dvh, dtype=np.float64).reshape(vh_obs.size, -1)
    n_tan = dvh.shape[1]
    kept = np.isfinite(vh_obs)
    m_abs = np.abs(vh_model)
    counted = kept & ~np.isnan(m_abs)
    s = float(wave_order_sum(lane_sums(np.where(counted, m_abs, 0.0))))
    n = float(wave_order_sum(lane_sums(counted.astype(np.float64))))
    n_kept = float(wave_order_sum(lane_sums(kept.astype(np.float64))))
    mean = s / n if n > 0.0 else NAN
    fill = (mean if mean > 100.0 else 100.0) if mean == mean else NAN
    m = np.where(np.isnan(vh_model), fill, vh_model)
    with np.errstate(invalid="ignore"):
        r = np.where(kept, vh_obs - m, 0.0)
    d = np.where(kept[:, None], dvh, 0.0)              # (a frequency outside K_i adds +0.0 to sums that start at +0.0)
    A = wave_order_sum(lane_sums(d[:, :, None] * d[:, None, :]))
    g = wave_order_sum(lane_sums(d * r[:, None]))
    cost = float(wave_order_sum(lane_sums(r * r)))
    return A, g, cost, n_kept, n_tan


def solve(A, g, lam, lambda_up):
    """(ok, delta, lam): the damped Cholesky step of lm_step, lambda raised while a pivot is not positive."""
    T = g.size
    for attempt in range(RETRIES + 1):
        if attempt > 0:
            lam = clamp(lam * lambda_up)
        L = np.zeros((T, T))
        ok = True
        for j in range(T):
            ajj = float(A[j, j])
            v = ajj + lam * (ajj if ajj > TINY else TINY)
            for m in range(j):
                v = v - L[j, m] * L[j, m]
            if not v > 0.0:
                ok = False
                break
            ljj = math.sqrt(v)
            L[j, j] = ljj
            for i in range(j + 1, T):
                u = float(A[i, j])
                for m in range(j):
                    u = u - L[i, m] * L[j, m]
                L[i, j] = u / ljj
        if ok:
            break
    if not ok:
        return False, None, lam
    y = np.zeros(T)
    for i in range(T):
        v = float(g[i])
        for m in range(i):
            v = v - L[i, m] * y[m]
        y[i] = v / L[i, i]
    delta = np.zeros(T)
    for i in range(T - 1, -1, -1):
        v = float(y[i])
        for m in range(i + 1, T):
            v = v - L[m, i] * delta[m]
        delta[i] = v / L[i, i]
    return True, delta, lam


def fit(evaluate, vh_obs, n_tan, c0=None, prior_weight=None, trace=None, **options):
    """One ionogram.  ``evaluate(c) -> (vh (F,), dvh (F, T))``.  Returns a dict: c, cost, status, n_eval, n_accept, lam,
    vh, history (max_iter,), A, g, delta.  ``trace``: a list that receives ``(c, c_eval, cost, lam, status)`` after
    every evaluation."""
    o = dict(DEFAULTS, **options)
    w = None if prior_weight is None else np.asarray(prior_weight, dtype=np.float64)
    vh_obs = np.asarray(vh_obs, dtype=np.float64)
    c = np.zeros(n_tan) if c0 is None else np.array(c0, dtype=np.float64)
    c_eval = c.copy()
    A, g, delta = np.zeros((n_tan, n_tan)), np.zeros(n_tan), np.zeros(n_tan)
    cost, lam = NAN, clamp(o["lambda0"])
    status, n_eval, n_accept = RUNNING, 0, 0
    vh_fit = np.full(vh_obs.size, NAN)
    history = np.full(o["max_iter"], NAN)
    for k in range(o["max_iter"]):
        if status != RUNNING:
            history[k] = cost
            continue
        vh, dvh = evaluate(c_eval.copy())
        eA, eg, ecost, n_kept, _ = eval_sums(vh_obs, vh, dvh)
        n_eval = k + 1
        accept = False
        if not n_kept > 0.0:
            status, cost = NO_DATA, NAN
        else:
            cost_eval = ecost
            if w is not None:
                for t in range(n_tan):
                    cost_eval = cost_eval + (w[t] * c_eval[t]) * c_eval[t]
            cost_prev = cost
            accept = True
            if k > 0:
                accept = bool(cost_eval < cost_prev)
                lam = clamp(lam / o["lambda_down"] if accept else lam * o["lambda_up"])
            if accept:
                n_accept += 1
                cost, c, A, g = cost_eval, c_eval.copy(), eA.copy(), eg.copy()
                if w is not None:
                    for t in range(n_tan):
                        A[t, t] = A[t, t] + w[t]
                        g[t] = g[t] - w[t] * c[t]
                vh_fit = np.array(vh, dtype=np.float64)
            if k == 0 and not math.isfinite(cost):
                status = NO_COST
            elif k > 0 and accept and cost_prev - cost <= o["ftol"] * cost_prev:
                status = CONVERGED_F
        if status == RUNNING:
            ok, step, lam = solve(A, g, lam, o["lambda_up"])
            if ok:
                dmax = float(np.max(np.abs(step))) if np.all(step == step) else NAN
                ok = math.isfinite(dmax)
            if not ok:
                status = SINGULAR
            else:
                delta = step
                cmax = float(np.max(np.abs(c)))
                if dmax > o["step_max"]:
                    delta = delta * (o["step_max"] / dmax)
                    dmax = o["step_max"]
                if dmax <= o["xtol"] * (cmax + o["xtol"]):
                    status = CONVERGED_X
                else:
                    c_eval = c + delta
        history[k] = cost
        if trace is not None:
            trace.append((c.copy(), c_eval.copy(), cost, lam, status))
    return dict(c=c, cost=cost, status=status, n_eval=n_eval, n_accept=n_accept, lam=lam, vh=vh_fit, history=history,
                A=A, g=g, delta=delta)


def capped_run(trace, step_max):
    """The longest run of consecutive evaluations of a ``trace`` of ``fit`` whose step was scaled to ``step_max``: the
    rule went on, and max |c_eval - c| equals ``step_max`` within an ulp of the largest number in the sum c + delta
    (the step itself is not in the trace; c_eval = fl(c + delta) is within half an ulp of c_eval of the sum, and delta's
    largest entry within an ulp of step_max)."""
    best = run = 0
    for c, c_eval, _, _, status in trace:
        size = float(np.max(np.abs(c_eval - c)))
        ulp = float(np.spacing(max(step_max, float(np.max(np.abs(c))), float(np.max(np.abs(c_eval))))))
        run = run + 1 if (status == RUNNING and abs(size - step_max) <= ulp) else 0
        best = max(best, run)
    return best
