"""The device Levenberg-Marquardt fit (prhf_vfo_lm_fit_f64) where tests/test_gpu_lm_fit.py does
not look: every basis size T = 1 ... 8, masks over several trips per lane, modelled NaN that are filled, the rule's rare
ends (SINGULAR, both clamps of lambda, the step cap, NO_DATA and NO_COST alone), tangents that go through the JVP in
chunks of 4, 2 and 1 (1000 - 1300 levels), and the ABI's strides longer than a row.

The method is that file's: tests/lm_rule.py - held to pyrayhf_amd/csrc/prhf_lm_step.h by tests/test_lm_fit_host.py -
driven by the device's own ``vh`` and ``dvh`` (``lm_cases.device_evaluate``) reproduces the kernel's whole state, so
every comparison here is of equal bits unless it says otherwise, and the two that are not derive their bounds.
Columns of fixture g26 (tests/lm_cases.py); observations from the CPU oracle; the cases are screened here at import,
on the CPU, and a case that fails its screen is an error of this file."""

import numpy as np
import pytest

import lm_rule
from conftest import same_bits
from lm_cases import (FIELDS, U, assert_the_rules_state, centres_of, column, device_evaluate, fit_case, gauss_basis,
                      native_fit, native_fit_case, oracle, state_of, well_posed)
from pyrayhf_amd import _native, fitting, library

pytestmark = pytest.mark.gpu

CONVERGED = (fitting.LM_CONVERGED_F, fitting.LM_CONVERGED_X)
BANDS = {"g": (0.01, 0.6), "d": (0.37, 0.6)}        # the well-posed bands of tests/test_gpu_lm_fit.py


def rule(w, obs=None, one_tangent_at_a_time=False, trace=None, **kw):
    """tests/lm_rule.py on the case ``w`` (its own observations, or ``obs``), driven by the device's vh and dvh."""
    obs = w["obs"] if obs is None else obs
    return lm_rule.fit(device_evaluate(dict(w, obs=obs), one_tangent_at_a_time), obs, w["B"].shape[0], trace=trace, **kw)


def numpy_products(dvh, res, kept):
    """``(A, its bound, g, its bound)``: d^T d and d^T r over the kept frequencies in plain NumPy, and the bounds of
    tests/test_gpu_lm_fit.py on sums of n_freq rounded products in any order, n_freq U |d|^T |.|."""
    d, r, n = dvh[kept], res[kept], dvh.shape[0]
    return d.T @ d, n * U * (np.abs(d).T @ np.abs(d)), d.T @ r, n * U * (np.abs(d).T @ np.abs(r))


# ---- 1. every basis size: lm_step_kernel<1> ... <8> ----

SIZES = {(name, T): well_posed(name, *BANDS[name], 100 + T, centres=centres_of(T), max_gap=None)
         for name in "gd" for T in range(1, 9)}


@pytest.mark.parametrize("n_tan", range(1, 9))
@pytest.mark.parametrize("name", ["g", "d"])
def test_every_basis_size_is_the_restated_rules(name, n_tan):
    """The lower triangle's indexing, the expansion to ``state`` and - inside the fit - the JVP's remainder rule (T = 5,
    6, 7 run on its instantiation for 8 tangents) depend on T: the full state after 1 and after 4 evaluations, without
    and with a prior, is the restated rule's; A is symmetric to the bit; and after one evaluation A and g are NumPy's
    d^T d and d^T r of ``library.vertical_jvp`` within the bounds of a sum of F rounded products."""
    w = SIZES[name, n_tan]
    assert w["B"].shape[0] == n_tan
    for prior in (None, np.linspace(0.0, 400.0, n_tan)):
        for max_iter in (1, 4):
            r = fit_case(w, prior_weight=prior, max_iter=max_iter, return_history=True, return_state=True)
            assert_the_rules_state(r, 0, rule(w, prior_weight=prior, max_iter=max_iter), (name, n_tan, prior is not None, max_iter))
            A, g, _ = state_of(r, 0, n_tan)
            assert np.array_equal(A, A.T) and np.isfinite(r.state).all()
            if prior is None and max_iter == 1:
                vh, dvh = library.vertical_jvp(w["f"], w["den"], w["bmag"], w["bpsi"], w["alt"], w["den"][None, :] * w["B"],
                                               w["mode"], w["n_points"])
                assert np.isfinite(vh).all() and dvh.shape == (10, n_tan)
                A_ref, A_bound, g_ref, g_bound = numpy_products(dvh, w["obs"] - vh, np.ones(10, dtype=bool))
                print(f"{name} T={n_tan}: max |A - d^T d| / bound {np.max(np.abs(A - A_ref) / A_bound):.3f}, "
                      f"max |g - d^T r| / bound {np.max(np.abs(g - g_ref) / g_bound):.3f}")
                assert np.all(np.abs(A - A_ref) <= A_bound) and np.all(np.abs(g - g_ref) <= g_bound)


# ---- 2. masks over several trips per lane ----

def masked_case():
    col = column("g")
    f = np.linspace(0.3, 0.6, 130) * col["freq"].max()
    B = gauss_basis(col["alt"], col["den"], centres_of(5))
    c_true = np.random.default_rng(5).uniform(-0.08, 0.08, 5)
    start = oracle(f, col["den"], col)[0]
    full = oracle(f, col["den"] * np.exp(c_true @ B), col)[0]
    assert np.isfinite(start).all() and np.isfinite(full).all()                     # the screen: every frequency reflects
    idx = np.arange(130)
    gone = (idx % 64 == 5) | np.isin(idx, (0, 63, 64, 127, 128, 129))               # lane 5 is empty on all its trips
    rest = np.nonzero(~gone)[0]
    gone[np.random.default_rng(130).choice(rest, rest.size // 5, replace=False)] = True     # a seeded 20 % of the rest
    obs = np.where(gone, np.nan, full)
    one = np.full(130, np.nan)
    one[129] = full[129]
    return dict(col, name="g", f=f, B=B, obs=obs), np.stack([obs, one])


MASKED, MASKED_OBS = masked_case()


@pytest.mark.parametrize("max_iter", [1, 5])
def test_masks_over_several_trips_per_lane_are_the_restated_rules(max_iter):
    """F = 130: lanes 0 and 1 make three trips, the others two; a frequency without an observation stays on its own
    lane, in both loops of the kernel.  The second ionogram of the call keeps f = 129 alone (lane 1, third trip)."""
    w = MASKED
    r = fitting.fit_profiles_lm(w["f"], MASKED_OBS, w["den"], w["bmag"], w["bpsi"], w["alt"], w["B"], w["mode"], w["n_points"],
                                max_iter=max_iter, return_history=True, return_state=True)
    for i in range(2):
        assert_the_rules_state(r, i, rule(w, obs=MASKED_OBS[i], max_iter=max_iter), (i, max_iter))
    assert np.isfinite(r.cost).all() and np.all(r.n_eval >= 1)


# ---- 3. fills: a frequency with an echo that the model does not reflect ----

def fill_case(name):
    col = column(name)
    f = np.linspace(0.3, 1.0, 130) * col["freq"].max()
    B = gauss_basis(col["alt"], col["den"], centres_of(5))
    start = oracle(f, col["den"], col)[0]
    obs = oracle(f, col["den"] * np.exp(np.full(5, 0.08) @ B), col)[0]
    filled, masked, ordinary = np.isfinite(obs) & np.isnan(start), np.isnan(obs), np.isfinite(obs) & np.isfinite(start)
    assert filled.sum() >= 4 and masked.sum() >= 20 and ordinary.sum() >= 40, (name, filled.sum(), masked.sum(), ordinary.sum())
    return dict(col, name=name, f=f, B=B, obs=obs, start=start, filled=filled)


FILLS = {name: fill_case(name) for name in "gd"}


@pytest.mark.parametrize("max_iter", [1, 6])
@pytest.mark.parametrize("name", ["g", "d"])
def test_fills_are_the_restated_rules_and_the_documented_cost(name, max_iter):
    """The truth (c = +0.08 on every direction) reflects eight frequencies that the start column does not: they are kept,
    their modelled NaN is filled with max(mean of the finite |vh| on K, 100 km), and their JVP rows are zero.
    (a) the state is the restated rule's; (b) after one evaluation the filled rows of dvh are exact zeros and A, g are
    NumPy's products over K with the fill applied; (c) the cost is ``residual_VH_many``'s on the result's column within
    the documented F 2^-52 cost; (d) the cost is a ``np.longdouble`` restatement's from the result's trace, within

        sum over K of (n + 3) U r_f^2  +  sum over the filled f of 2 |r_f| F U fill,   U = 2^-52, n = ceil(F / 64) + 6:

    r_f = fl(o - m) and fl(r_f r_f) are two roundings, the term enters a lane's sum of at most ceil(F / 64) additions
    and the tree's 6: (1 + U/2)^(n + 3) - 1 < (n + 3) U of the term.  The fill is a sum of at most F positive terms
    through n additions and one division, so it is within (n + 1) U / 2 < F U of the mean, relatively; a filled
    residual moves by that much, its square by 2 |r_f| times it (the square of the move is below the bound's slack:
    the roundings above are counted at U, twice their size)."""
    w = FILLS[name]
    n_freq, kept = w["f"].size, np.isfinite(w["obs"])
    r = fit_case(w, max_iter=max_iter, return_history=True, return_state=True)
    if max_iter == 1:
        # the device's model is the oracle's at every frequency: the grid does not sit on a cusp
        assert np.array_equal(np.isnan(r.vh[0]), np.isnan(w["start"]))
    # (a)
    assert_the_rules_state(r, 0, rule(w, max_iter=max_iter), (name, max_iter))
    assert np.isfinite(r.cost[0]) and np.isfinite(r.state).all()
    # (d), and the fill for (b)
    vh = r.vh[0]
    filled = kept & np.isnan(vh)
    counted = kept & ~np.isnan(vh)
    fill = max(float(np.mean(np.abs(vh[counted]).astype(np.longdouble))), 100.0)
    res = np.where(kept, w["obs"] - np.where(np.isnan(vh), fill, vh), 0.0)
    exact = float(np.sum(res[kept].astype(np.longdouble) ** 2))
    n = -(-n_freq // 64) + 6
    bound = float(np.sum((n + 3) * U * res[kept] ** 2) + np.sum(2.0 * np.abs(res[filled]) * n_freq * U * fill))
    print(f"{name} max_iter={max_iter}: {int(filled.sum())} filled of {int(kept.sum())} kept, fill {fill:.3f} km, cost "
          f"{r.cost[0]:.6e}, |cost - longdouble| / bound {abs(r.cost[0] - exact) / bound:.3f}")
    assert abs(r.cost[0] - exact) <= bound
    # (c)
    cost, _, _ = fitting.residual_VH_many(w["f"], w["obs"][None, :], r.den, w["bmag"], w["bpsi"], w["alt"], w["mode"],
                                          w["n_points"], ionogram_of_row=np.zeros(1, dtype=np.int32))
    print(f"{name} max_iter={max_iter}: residual_VH_many {cost[0]:.6e}, difference / (F U cost) "
          f"{abs(r.cost[0] - cost[0]) / (n_freq * U * cost[0]):.3f}")
    assert abs(r.cost[0] - cost[0]) <= n_freq * U * cost[0]
    # (b)
    if max_iter == 1:
        assert filled.sum() >= 4 and np.array_equal(filled, w["filled"])
        vh0, dvh = library.vertical_jvp(w["f"], w["den"], w["bmag"], w["bpsi"], w["alt"], w["den"][None, :] * w["B"],
                                        w["mode"], w["n_points"])
        assert same_bits(vh0, vh) and np.all(dvh[np.isnan(vh)] == 0.0)
        A, g, _ = state_of(r, 0, 5)
        A_ref, A_bound, g_ref, g_bound = numpy_products(dvh, res, kept)
        assert np.all(np.abs(A - A_ref) <= A_bound) and np.all(np.abs(g - g_ref) <= g_bound)


# ---- 4. the rare ends, through the native call ----

WELL_G = well_posed("g", *BANDS["g"], 26)            # T = 3, the well-posed case g of tests/test_gpu_lm_fit.py


def test_singular_after_eight_retries_and_the_neighbour_untouched():
    """The basis times 2^k: the rows of dvh stay finite and d^T d overflows, so the factor's first column is inf / inf
    and no pivot is positive at any lambda: eight retries, SINGULAR at the first evaluation with lambda0 10^8 = 1e5, no
    step.  k: the first of a short list, 520 at its head, at which ``library.vertical_jvp`` at c0 shows both."""
    w = WELL_G
    for k in (520, 524, 516, 528, 512):
        huge = dict(w, B=w["B"] * 2.0 ** k)
        vh, dvh = library.vertical_jvp(w["f"], w["den"], w["bmag"], w["bpsi"], w["alt"], w["den"][None, :] * huge["B"], w["mode"],
                                       w["n_points"])
        with np.errstate(over="ignore", invalid="ignore"):
            if np.isfinite(dvh).all() and np.isinf(np.diag(dvh.T @ dvh)).all():
                break
    else:
        raise AssertionError("no k leaves dvh finite with an overflowing d^T d")
    print(f"k = {k}: max |dvh| = {np.max(np.abs(dvh)):.3e}")
    both = np.ascontiguousarray(np.stack([huge["B"], w["B"]]))
    obs2 = np.ascontiguousarray(np.stack([w["obs"], w["obs"]]))
    r = native_fit(w["f"], obs2, w["den"], w["bmag"], w["bpsi"], w["alt"], both, w["mode"], w["n_points"])
    assert (r.status[0], r.n_eval[0], r.n_accept[0]) == (fitting.LM_SINGULAR, 1, 1)
    assert abs(r.lam[0] - 1e5) <= 4 * np.spacing(1e5) and np.array_equal(state_of(r, 0, 3)[2], np.zeros(3))
    assert same_bits(r.c[0], np.zeros(3)) and np.isfinite(r.cost[0])
    assert np.max(np.abs(r.den[0] - w["den"]) / w["den"]) <= 1e-14 and same_bits(r.vh[0], vh)
    with np.errstate(over="ignore", invalid="ignore"):
        assert_the_rules_state(r, 0, rule(huge), "singular")
    # one ionogram's overflow does not touch the next
    alone = native_fit_case(w)
    assert alone.status[0] in CONVERGED
    for name in FIELDS:
        assert same_bits(getattr(r, name)[1], getattr(alone, name)[0]), name


def test_rounding_floor_reaches_both_clamps_of_lambda():
    """ftol = xtol = 0, lambda_up = 1e3, lambda_down = 1e6, 40 evaluations: nothing ends the fit; accepted steps take
    lambda to 1e-12, and once the cost stops falling the rejections take it to 1e12."""
    w = WELL_G
    options = dict(ftol=0.0, xtol=0.0, lambda_up=1e3, lambda_down=1e6, max_iter=40)
    r = native_fit_case(w, **options)
    trace = []
    assert_the_rules_state(r, 0, rule(w, trace=trace, **options), "floor")
    lams = [t[3] for t in trace]
    print("lambda after every evaluation:", " ".join(f"{v:g}" for v in lams))
    assert r.status[0] == fitting.LM_RUNNING and r.n_eval[0] == 40
    assert np.all(np.diff(r.cost_history[0]) <= 0.0)
    assert lm_rule.LAMBDA_MAX in lams and r.lam[0] == lams[-1]


def test_step_cap_scales_the_first_steps():
    w = WELL_G
    r = native_fit_case(w, step_max=0.01, max_iter=8)
    trace = []
    assert_the_rules_state(r, 0, rule(w, trace=trace, step_max=0.01, max_iter=8), "cap")
    print("max |c_eval - c| after every evaluation:", " ".join(f"{np.max(np.abs(t[1] - t[0])):.17g}" for t in trace))
    assert lm_rule.capped_run(trace, 0.01) >= 3


def no_cost_case():
    """Case g with two frequencies above the start column's critical frequency, and echoes on those two only."""
    w = WELL_G
    f = np.concatenate([w["f"], np.array([1.3, 1.4]) * w["freq"].max()])
    c0 = np.array([0.01, 0.0, -0.01])
    start = oracle(f, w["den"] * np.exp(c0 @ w["B"]), w)[0]
    assert np.isnan(start[10:]).all() and np.isfinite(start[:10]).all()             # the screen
    obs = np.concatenate([np.full(10, np.nan), [300.0, 300.0]])
    return dict(w, f=f, obs=obs), c0


NO_COST, NO_COST_C0 = no_cost_case()


def test_no_data_and_no_cost_alone_are_the_restated_rules():
    """Each alone in its call, with history, against the rule and not against a batch.  NO_COST: no kept frequency has
    a modelled height, the fill and the cost are NaN; its column is the finite one at c0 and its trace the operator's.
    NO_DATA: no observation; c is c0, the column and the trace are NaN."""
    w, c0 = NO_COST, NO_COST_C0
    r = native_fit_case(w, c0=np.ascontiguousarray(c0[None, :]), max_iter=3)
    assert (r.status[0], r.n_eval[0], r.n_accept[0]) == (fitting.LM_NO_COST, 1, 1) and np.isnan(r.cost[0])
    with np.errstate(invalid="ignore"):
        assert_the_rules_state(r, 0, rule(w, c0=c0, max_iter=3), "no cost")
    want = w["den"] * np.exp(c0 @ w["B"])
    assert np.max(np.abs(r.den[0] - want) / want) <= 1e-14
    assert np.isfinite(r.vh[0, :10]).all() and np.isnan(r.vh[0, 10:]).all() and same_bits(r.c[0], c0)

    nothing = np.full(12, np.nan)
    r = native_fit_case(w, obs=nothing, c0=np.ascontiguousarray(c0[None, :]), max_iter=3)
    # (the rule evaluates before it looks at the data: its column comes from a fit that has some)
    want = lm_rule.fit(device_evaluate(dict(w, obs=np.full(12, 300.0))), nothing, 3, c0=c0, max_iter=3)
    assert want["status"] == lm_rule.NO_DATA and (r.n_eval[0], r.n_accept[0]) == (1, 0)
    assert_the_rules_state(r, 0, want, "no data")
    assert np.isnan(r.den[0]).all() and np.isnan(r.vh[0]).all() and np.isnan(r.cost[0]) and same_bits(r.c[0], c0)
    assert np.isnan(r.cost_history[0]).all()


# ---- 5. tangents in chunks of 4, 2 and 1 inside the fit ----

def padded_o(n_alt, n_tan):
    """Column o (620 levels) padded above its peak to ``n_alt`` levels, as the tall case of tests/test_gpu_lm_fit.py
    pads it; T directions, 10 frequencies, the oracle's trace of a perturbed column o."""
    col = column("o")
    f = (np.linspace(0.3, 0.6, 130) * col["freq"].max())[np.round(np.linspace(0, 129, 10)).astype(int)]
    B = gauss_basis(col["alt"], col["den"], centres_of(n_tan))
    c_true = np.random.default_rng(n_alt).uniform(-0.08, 0.08, n_tan)
    obs = oracle(f, col["den"] * np.exp(c_true @ B), col)[0]
    assert np.isfinite(obs).all()
    extra = n_alt - col["alt"].size
    step = col["alt"][-1] - col["alt"][-2]
    w = dict(col, name="o", f=f, obs=obs)
    w["alt"] = np.concatenate([col["alt"], col["alt"][-1] + step * np.arange(1, extra + 1)])
    w["den"] = np.concatenate([col["den"], col["den"][-1] * np.exp(-np.arange(1, extra + 1) / 50.0)])
    w["bmag"] = np.concatenate([col["bmag"], np.full(extra, col["bmag"][-1])])
    w["bpsi"] = np.concatenate([col["bpsi"], np.full(extra, col["bpsi"][-1])])
    w["B"] = np.concatenate([B, np.zeros((n_tan, extra))], axis=1)
    assert int(np.argmax(w["den"])) == int(np.argmax(col["den"])) and w["alt"].size == n_alt
    return w


TALL = {(n_alt, n_tan): padded_o(n_alt, n_tan) for n_alt, n_tan in ((1000, 8), (1200, 5), (1300, 3))}


@pytest.mark.parametrize("n_alt, n_tan", list(TALL))
def test_chunked_tangents_inside_the_fit(n_alt, n_tan):
    """n_alt <= 1332, so the whole padded column is staged and the JVP's plan (plan_jvp, prhf_plan.h; printed by
    tests/devtools/jvp_plan_host.cpp) takes the tangents in chunks: 1000 levels, T = 8: 2 launches of 4; 1200 levels,
    T = 5: 3 launches of 2, 2 and 1; 1300 levels, T = 3: 3 launches of 1.  ``jvp_run`` advances the ``dvh`` column per
    chunk inside the fit's (I, F, T) layout.  The rule is driven by ``library.vertical_jvp`` on the same padded column
    ONE tangent per call - a plan of one chunk, column 0 - so a chunk written at the wrong offset cannot be on both
    sides; the call with all T at once gives the same bits.
    The counters: a timed launch is one pair of events (prhf_recent_kernel_ms), and the chunks of one JVP share a
    pair - four per evaluation and the last column's at every height, 3 x 4 + 1 - and nothing waits but the end."""
    w = TALL[n_alt, n_tan]
    fit_case(w, max_iter=3)                                   # (the context's buffers take their size)
    r = fit_case(w, max_iter=3, return_history=True, return_state=True)
    assert _native.host_context(0).lm_fit_counters() == (3, 3 * 4 + 1, 1)
    assert_the_rules_state(r, 0, rule(w, one_tangent_at_a_time=True, max_iter=3), (n_alt, n_tan))
    vh, dvh = device_evaluate(w)(np.zeros(n_tan))
    vh1, dvh1 = device_evaluate(w, one_tangent_at_a_time=True)(np.zeros(n_tan))
    assert same_bits(vh, vh1) and same_bits(dvh, dvh1) and np.all(np.any(dvh != 0.0, axis=0))
    assert np.isfinite(r.state).all() and r.n_eval[0] == 3


# ---- 6. strides longer than a row ----

def test_strides_longer_than_a_row_equal_the_packed_call():
    """Three ionograms (columns g, h, d on their common altitudes, X mode), den0 rows at stride n_alt + 5 and basis sets
    at stride T n_alt + 7, the gaps NaN: the host route compacts them (put_rows), the device route reads them in place
    (lm_synth_kernel) and also takes per-ionogram altitude rows at stride n_alt + 3.  Every output is the packed call's."""
    import torch
    cols = [column(n) for n in "ghd"]
    alt = cols[0]["alt"]
    assert all(np.array_equal(c["alt"], alt) for c in cols)
    n_alt, n_tan, n_iono = alt.size, 3, 3
    f = np.linspace(0.37, 0.6, 10) * cols[2]["freq"].max()
    den0 = np.stack([c["den"] for c in cols])
    bmag, bpsi = np.stack([c["bmag"] for c in cols]), np.stack([c["bpsi"] for c in cols])
    B = np.stack([gauss_basis(alt, c["den"], (0.25, 0.575, 0.9)) for c in cols])
    c_true = np.random.default_rng(3).uniform(-0.08, 0.08, (n_iono, n_tan))
    obs = np.stack([oracle(f, den0[i] * np.exp(c_true[i] @ B[i]), cols[i], "X", 64)[0] for i in range(n_iono)])
    assert np.isfinite(obs).all()
    obs[1, 4] = np.nan
    prior = np.array([0.0, 1.0, 10.0])
    kw = dict(prior=prior, max_iter=6)
    packed = native_fit(f, obs, den0, bmag, bpsi, alt, B, "X", 64, **kw)
    assert np.isfinite(packed.cost).all() and np.all(packed.n_eval >= 2)

    den0_wide = np.full((n_iono, n_alt + 5), np.nan)
    den0_wide[:, :n_alt] = den0
    B_wide = np.full((n_iono, n_tan * n_alt + 7), np.nan)
    B_wide[:, :n_tan * n_alt] = B.reshape(n_iono, -1)
    alt_wide = np.full((n_iono, n_alt + 3), np.nan)
    alt_wide[:, :n_alt] = alt
    strides = dict(n_alt=n_alt, n_tan=n_tan, den0_stride=n_alt + 5, basis_stride=n_tan * n_alt + 7)
    host = native_fit(f, obs, den0_wide, bmag, bpsi, alt, B_wide, "X", 64, **strides, **kw)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(x, device=dev)             # noqa: E731
    device = native_fit(t(f), t(obs), t(den0_wide), t(bmag), t(bpsi), t(alt_wide), t(B_wide), "X", 64, alt_stride=n_alt + 3,
                        **strides, prior=t(prior), max_iter=6)
    for name in FIELDS:
        assert same_bits(getattr(host, name), getattr(packed, name)), ("host", name)
        assert same_bits(getattr(device, name).cpu().numpy(), getattr(packed, name)), ("device", name)
