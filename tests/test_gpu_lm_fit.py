"""Levenberg-Marquardt fits of many ionograms on the device (prhf_vfo_lm_fit_f64, ``fitting.fit_profiles_lm``,
DESIGN.md section 4.16) on columns of fixture g26: the 78-level columns g (O mode), h and d (X mode), the 620-level o.

Basis: Gaussian bumps of width 0.2 in the normalised bottomside height z = (alt - alt[0]) / (hmF2 - alt[0]); T = 3 with
centres 0.25, 0.575, 0.9 for the well-posed cases; T = 1 (centre 0.575) and T = 8 join them for the arithmetic.  Truth: |c_t| <= 0.08.
Observations: the CPU oracle (oracle/vfo_numpy.py) on den0 exp(c_true B) - never the code under test.  The well-posed
cases keep their 10 frequencies away from the cusps (g: 0.01 - 0.6 x the fixture's highest frequency, h and d: 0.37 -
0.6 x) and are screened here, at import, on the CPU: every frequency reflects for the start and for the truth, and
max |vh_start - vh_obs| <= 25 km.  A case that fails the screen is an error of this file.

The host route of the recovery test is tests/lm_rule.py driven by ``library.vertical_jvp`` - pinned code, not the code
under test; its figures go to profiles/lm_fit_parity.md and set the bounds (10 x the host route's)."""

import os

import numpy as np
import pytest

import lm_rule
from conftest import REPO, same_bits
from lm_cases import CENTRES3, FIELDS, U, column, device_evaluate, fit_case, gauss_basis, oracle, well_posed
from oracle import vfo_numpy as orc
from parity_report import put_section
from pyrayhf_amd import _native, fitting, library

pytestmark = pytest.mark.gpu

PARITY = os.path.join(REPO, "profiles", "lm_fit_parity.md")
CONVERGED = (fitting.LM_CONVERGED_F, fitting.LM_CONVERGED_X)

WELL = {"g": well_posed("g", 0.01, 0.6, 26), "h": well_posed("h", 0.37, 0.6, 27), "d": well_posed("d", 0.37, 0.6, 28)}


# ---- 1. one step is the NumPy step ----

@pytest.fixture(scope="module")
def arithmetic_cases():
    """name -> (column, basis, 130 frequencies, the oracle's trace of a perturbed column on them)."""
    out = {}
    for name, centres, band in (("g", CENTRES3, (0.3, 0.6)), ("g1", (0.575,), (0.3, 0.6)),
                                ("o", np.linspace(0.1, 0.95, 8), (0.3, 0.6))):
        col = column(name[0])
        f = np.linspace(*band, 130) * col["freq"].max()
        B = gauss_basis(col["alt"], col["den"], centres)
        c_true = np.random.default_rng(len(centres)).uniform(-0.08, 0.08, len(centres))
        obs = oracle(f, col["den"] * np.exp(c_true @ B), col)[0]
        assert np.isfinite(obs).all()
        out[name] = (col, B, f, obs)
    return out


@pytest.mark.parametrize("n_freq", [1, 10, 64, 65, 130])
@pytest.mark.parametrize("name", ["g", "g1", "o"])          # T = 3, 1 and 8
def test_one_step_is_the_numpy_step(arithmetic_cases, name, n_freq):
    col, B, f, obs = arithmetic_cases[name]
    pick = np.round(np.linspace(0, 129, n_freq)).astype(int) if n_freq > 1 else np.array([64])
    f, obs = f[pick], obs[pick]
    T = B.shape[0]
    r = fitting.fit_profiles_lm(f, obs[None, :], col["den"], col["bmag"], col["bpsi"], col["alt"], B, col["mode"],
                                col["n_points"], max_iter=1, step_max=1e300, return_state=True)
    A = r.state[0, :T * T].reshape(T, T)
    g = r.state[0, T * T:T * T + T]
    delta = r.state[0, T * T + T:]
    vh, dvh = library.vertical_jvp(f, col["den"], col["bmag"], col["bpsi"], col["alt"], col["den"][None, :] * B, col["mode"],
                                   col["n_points"])
    assert np.isfinite(vh).all()                            # (every frequency reflects: no fill to apply)
    res = obs - vh
    A_ref = dvh.T @ dvh
    A_bound = n_freq * U * (np.abs(dvh).T @ np.abs(dvh))
    g_ref = dvh.T @ res
    g_bound = n_freq * U * (np.abs(dvh).T @ np.abs(res))
    print(f"{name} F={n_freq}: max |A - d^T d| / bound {np.max(np.abs(A - A_ref) / A_bound):.3f}, "
          f"max |g - d^T r| / bound {np.max(np.abs(g - g_ref) / g_bound):.3f}")
    assert np.all(np.abs(A - A_ref) <= A_bound)
    assert np.all(np.abs(g - g_ref) <= g_bound)
    assert np.array_equal(A, A.T)
    lam = float(r.lam[0])
    M = A + lam * np.diag(np.maximum(np.diag(A), 1e-30))
    back = np.max(np.abs(M @ delta - g))
    limit = 64 * U * (np.max(np.sum(np.abs(M), axis=1)) * np.max(np.abs(delta)) + np.max(np.abs(g)))
    print(f"{name} F={n_freq}: lambda {lam:g}, backward error {back:.3e}, limit {limit:.3e}")
    assert back <= limit
    assert r.status[0] == fitting.LM_RUNNING and r.n_eval[0] == 1 and r.n_accept[0] == 1
    assert same_bits(r.c[0], np.zeros(T)) and same_bits(r.vh[0], vh)
    assert r.cost[0] == pytest.approx(float(res @ res), rel=n_freq * U)


# ---- 2. consistency at the result ----

@pytest.fixture(scope="module")
def well_fits():
    return {name: fit_case(w, return_history=True) for name, w in WELL.items()}


@pytest.mark.parametrize("name", ["g", "h", "d"])
def test_consistency_at_the_result(well_fits, name):
    w, r = WELL[name], well_fits[name]
    vh = library.vertical_forward_operator(w["f"], r.den, np.broadcast_to(w["bmag"], r.den.shape).copy(),
                                           np.broadcast_to(w["bpsi"], r.den.shape).copy(), w["alt"], w["mode"], w["n_points"])
    assert same_bits(vh, r.vh)
    want = w["den"] * np.exp(r.c[0] @ w["B"])
    assert np.max(np.abs(r.den[0] - want) / want) <= 1e-14
    cost, _, _ = fitting.residual_VH_many(w["f"], w["obs"][None, :], r.den, w["bmag"], w["bpsi"], w["alt"], w["mode"],
                                          w["n_points"], ionogram_of_row=np.zeros(1, dtype=np.int32))
    print(f"{name}: cost {r.cost[0]:.6e}, residual_VH_many {cost[0]:.6e}")
    assert abs(r.cost[0] - cost[0]) <= w["f"].size * U * cost[0]


def test_consistency_with_a_prior(well_fits):
    w = WELL["g"]
    prior = np.array([0.0, 40.0, 400.0])
    r = fit_case(w, prior_weight=prior)
    cost, _, _ = fitting.residual_VH_many(w["f"], w["obs"][None, :], r.den, w["bmag"], w["bpsi"], w["alt"], w["mode"],
                                          w["n_points"], ionogram_of_row=np.zeros(1, dtype=np.int32))
    total = cost[0] + float(np.sum(prior * r.c[0] ** 2))
    assert abs(r.cost[0] - total) <= (w["f"].size + 3) * U * total
    assert np.max(np.abs(r.c[0])) <= np.max(np.abs(well_fits["g"].c[0]))


# ---- 3. descent ----

def check_descent(r, max_iter):
    h = r.cost_history
    assert h.shape == (r.c.shape[0], max_iter)
    assert np.all(np.diff(h, axis=1) <= 0.0), h
    assert np.all(r.n_accept <= r.n_eval) and np.all(r.n_eval <= max_iter) and np.all(r.n_accept >= 1)
    assert same_bits(h[:, -1], r.cost)


@pytest.mark.parametrize("name", ["g", "h", "d"])
def test_descent_on_the_well_posed_cases(well_fits, name):
    check_descent(well_fits[name], 20)


def test_descent_on_an_ill_posed_basis_with_and_without_a_prior():
    w = WELL["g"]
    B = gauss_basis(w["alt"], w["den"], np.linspace(0.1, 0.95, 8))
    w8 = dict(w, B=B)
    free = fit_case(w8, return_history=True)
    check_descent(free, 20)
    tied = fit_case(w8, return_history=True, prior_weight=np.full(8, 100.0))
    check_descent(tied, 20)
    print(f"T = 8, F = 10: max |c| {np.max(np.abs(free.c)):.3e} without a prior, {np.max(np.abs(tied.c)):.3e} with; "
          f"cost {free.cost[0]:.3e} / {tied.cost[0]:.3e}, status {free.status[0]} / {tied.status[0]}")
    assert np.max(np.abs(tied.c)) < np.max(np.abs(free.c))


# ---- 4. recovery ----

def host_route(w, max_iter=20):
    """tests/lm_rule.py driven by ``library.vertical_jvp``: one call per evaluation, the step on the host."""
    def evaluate(c):
        den = w["den"] * np.exp(c @ w["B"])
        return library.vertical_jvp(w["f"], den, w["bmag"], w["bpsi"], w["alt"], den[None, :] * w["B"], w["mode"], w["n_points"])
    return lm_rule.fit(evaluate, w["obs"], w["B"].shape[0], max_iter=max_iter)


@pytest.fixture(scope="module")
def host_fits():
    fits = {name: host_route(w) for name, w in WELL.items()}
    lines = ["# Levenberg-Marquardt fit: the host route on the screened cases",
             "",
             "tests/lm_rule.py driven by `library.vertical_jvp`, 10 frequencies, T = 3, start 0, at most 20 evaluations "
             "(tests/test_gpu_lm_fit.py writes this table; its recovery bounds are 10 x these figures).",
             "",
             "| case | mode | start cost | final cost / start cost | max abs(c - c_true) | status | evaluations |",
             "|---|---|---|---|---|---|---|"]
    for name, r in fits.items():
        w = WELL[name]
        lines.append(f"| {name} | {w['mode']} | {r['history'][0]:.6e} | {r['cost'] / r['history'][0]:.3e} | "
                     f"{np.max(np.abs(r['c'] - w['c_true'])):.3e} | {fitting.LM_STATUS_NAMES[r['status']]} | {r['n_eval']} |")
    put_section(lines, PARITY)
    print("\n".join(lines))
    return fits


@pytest.mark.parametrize("name", ["g", "h", "d"])
def test_recovery_within_ten_times_the_host_route(well_fits, host_fits, name):
    w, r, host = WELL[name], well_fits[name], host_fits[name]
    ratio, err = r.cost[0] / r.cost_history[0, 0], np.max(np.abs(r.c[0] - w["c_true"]))
    host_ratio, host_err = host["cost"] / host["history"][0], np.max(np.abs(host["c"] - w["c_true"]))
    print(f"{name}: device cost ratio {ratio:.3e} (host {host_ratio:.3e}), max |c - c_true| {err:.3e} (host {host_err:.3e}), "
          f"status {fitting.LM_STATUS_NAMES[int(r.status[0])]} after {r.n_eval[0]} evaluations (host {host['n_eval']})")
    assert r.status[0] in CONVERGED and r.n_eval[0] <= 20
    assert same_bits(r.cost_history[0, 0], host["history"][0])      # the same evaluation at the start
    assert ratio <= 10.0 * host_ratio
    assert err <= 10.0 * host_err


# ---- 5. batch independence ----

N_BATCH = 67
NO_DATA_AT, NO_COST_AT = 5, 11          # (11 % 3 == 2: a column of case d, whose critical frequency is the lower one)


@pytest.fixture(scope="module")
def batch():
    cols = [column(n) for n in "ghd"]
    alt = cols[0]["alt"]
    assert all(np.array_equal(c["alt"], alt) for c in cols)
    top = cols[2]["freq"].max()                              # case d's highest fixture frequency, the lowest of the three
    f = np.concatenate([np.linspace(0.37, 0.6, 10) * top, [1.3 * top, 1.4 * top]])
    rng = np.random.default_rng(67)
    pick = [cols[i % 3] for i in range(N_BATCH)]
    den0 = np.stack([c["den"] for c in pick])
    bmag, bpsi = np.stack([c["bmag"] for c in pick]), np.stack([c["bpsi"] for c in pick])
    B = np.stack([gauss_basis(alt, c["den"], CENTRES3) for c in pick])
    c_true = rng.uniform(-0.08, 0.08, (N_BATCH, 3))
    truth = den0 * np.exp(np.einsum("it,itk->ik", c_true, B))
    obs = orc.virtual_heights_batch(f, truth, bmag, bpsi, alt, "X", 64)
    obs[NO_DATA_AT] = np.nan
    start = orc.virtual_heights_batch(f, den0[NO_COST_AT:NO_COST_AT + 1], bmag[NO_COST_AT:NO_COST_AT + 1],
                                      bpsi[NO_COST_AT:NO_COST_AT + 1], alt, "X", 64)[0]
    assert np.isnan(start[10:]).all() and np.isfinite(start[:10]).all()     # the two highest escape the start profile
    obs[NO_COST_AT, :10] = np.nan
    obs[NO_COST_AT, 10:] = 300.0
    args = dict(freq=f, vh_obs=obs, den0=den0, bmag=bmag, bpsi=bpsi, alt=alt, basis=B, mode="X", n_points=64)
    return args, fitting.fit_profiles_lm(**args, return_history=True, return_state=True)


def test_batch_rows_equal_the_ionogram_fitted_alone(batch):
    args, r = batch
    assert r.status[NO_DATA_AT] == fitting.LM_NO_DATA and np.isnan(r.cost[NO_DATA_AT])
    assert np.isnan(r.den[NO_DATA_AT]).all() and np.isnan(r.vh[NO_DATA_AT]).all() and same_bits(r.c[NO_DATA_AT], np.zeros(3))
    assert r.status[NO_COST_AT] == fitting.LM_NO_COST and not np.isfinite(r.cost[NO_COST_AT])
    assert np.isin(r.status, CONVERGED).sum() >= N_BATCH // 2, r.status
    for i in range(N_BATCH):
        one = fitting.fit_profiles_lm(args["freq"], args["vh_obs"][i:i + 1], args["den0"][i], args["bmag"][i], args["bpsi"][i],
                                      args["alt"], args["basis"][i], "X", 64, return_history=True, return_state=True)
        for name in FIELDS:
            assert same_bits(getattr(r, name)[i], getattr(one, name)[0]), (i, name)


def test_frozen_means_frozen(batch):
    args, r = batch
    longer = fitting.fit_profiles_lm(**args, max_iter=40, return_history=True, return_state=True)
    done = r.status != fitting.LM_RUNNING
    assert np.isin(r.status, CONVERGED).any()
    for name in FIELDS[:-1]:
        assert same_bits(getattr(r, name)[done], getattr(longer, name)[done]), name
    assert same_bits(r.cost_history[done], longer.cost_history[done][:, :20])
    assert same_bits(longer.cost_history[done][:, 20:], np.repeat(r.cost[done][:, None], 20, axis=1))


# ---- 6. residency ----

def test_device_resident_inputs_one_synchronisation(batch):
    import torch
    args, r = batch
    dev = torch.device("cuda", 0)
    t = {k: torch.as_tensor(v, device=dev) for k, v in args.items() if isinstance(v, np.ndarray)}
    kw = dict(args, **t)
    fitting.fit_profiles_lm(**kw, return_history=True, return_state=True)               # (the context's buffers take their size)
    got = fitting.fit_profiles_lm(**kw, return_history=True, return_state=True)
    evaluations, launches, waits = _native.context(0).lm_fit_counters()
    assert (evaluations, launches, waits) == (20, 4 * 20 + 1, 1)      # 78 levels: the whole column fits the JVP's plan
    for name in FIELDS:
        v = getattr(got, name)
        assert torch.is_tensor(v) and v.device == dev, name
        assert same_bits(v.cpu().numpy(), getattr(r, name)), name


# ---- 7. shared and per-ionogram basis and field ----

def test_shared_arrays_equal_their_expansion():
    w = WELL["h"]
    rng = np.random.default_rng(7)
    n = 5
    obs = np.stack([w["obs"] + rng.normal(0.0, 0.5, w["obs"].size) for _ in range(n)])
    obs[2, 3] = np.nan
    c0 = rng.uniform(-0.02, 0.02, (n, 3))
    shared = fitting.fit_profiles_lm(w["f"], obs, w["den"], w["bmag"], w["bpsi"], w["alt"], w["B"], "X", w["n_points"], c0=c0,
                                     return_history=True, return_state=True)
    rows = lambda x: np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape))      # noqa: E731
    own = fitting.fit_profiles_lm(w["f"], obs, rows(w["den"]), rows(w["bmag"]), rows(w["bpsi"]), w["alt"], rows(w["B"]), "X",
                                  w["n_points"], c0=c0, return_history=True, return_state=True)
    mixed = fitting.fit_profiles_lm(w["f"][::-1].copy(), obs[:, ::-1].copy(), rows(w["den"]), w["bmag"], w["bpsi"], w["alt"],
                                    w["B"], "X", w["n_points"], c0=c0, return_history=True, return_state=True)
    for name in FIELDS:
        assert same_bits(getattr(shared, name), getattr(own, name)), name
        assert same_bits(getattr(shared, name), getattr(mixed, name)), name      # (columns follow the ascending grid)
    one_start = fitting.fit_profiles_lm(w["f"], obs, w["den"], w["bmag"], w["bpsi"], w["alt"], w["B"], "X", w["n_points"],
                                        c0=c0[0])
    assert same_bits(one_start.c[0], shared.c[0])


# ---- the state after many evaluations is the restated rule's, driven by the device's own vh and dvh ----

@pytest.mark.parametrize("prior", [None, (0.0, 40.0, 400.0)])
@pytest.mark.parametrize("name", ["g", "h", "d"])
def test_state_after_many_evaluations_is_the_restated_rules(name, prior):
    w = WELL[name]
    T = w["B"].shape[0]
    seen = set()
    for max_iter in (2, 5, 20):                              # a step kept, a rejection or two, and the frozen end
        r = fit_case(w, prior_weight=prior, max_iter=max_iter, return_history=True, return_state=True)
        want = lm_rule.fit(device_evaluate(w), w["obs"], T, prior_weight=prior, max_iter=max_iter)
        assert (int(r.status[0]), int(r.n_eval[0]), int(r.n_accept[0])) == (want["status"], want["n_eval"], want["n_accept"])
        assert same_bits(r.c[0], want["c"]) and same_bits(r.cost[0], want["cost"]) and same_bits(r.lam[0], want["lam"])
        assert same_bits(r.cost_history[0], want["history"]) and same_bits(r.vh[0], want["vh"])
        assert same_bits(r.state[0, :T * T].reshape(T, T), want["A"]), (name, max_iter)
        assert same_bits(r.state[0, T * T:T * T + T], want["g"]), (name, max_iter)
        assert same_bits(r.state[0, T * T + T:], want["delta"]), (name, max_iter)
        assert np.isfinite(r.state).all()
        seen.add(int(r.status[0]))
    # (coverage of the frozen end, not a property of the fit: the screened cases end within 20 evaluations - the recovery
    #  test demands it; with a prior term nothing says they do)
    assert prior is not None or seen & set(CONVERGED)


# ---- the entry's own argument checks ----

def test_bad_arguments_are_einval_from_the_entry():
    w = WELL["g"]
    ctx = _native.host_context(0)
    mult = library._multiplier(w["n_points"])
    n_alt, n_freq = w["alt"].size, w["f"].size
    obs = np.ascontiguousarray(w["obs"][None, :])
    B9 = np.ascontiguousarray(np.concatenate([w["B"]] * 3))
    out = dict(c=np.empty((1, 9)), cost=np.empty(1), status=np.empty(1, np.int32), n_eval=np.empty(1, np.int32),
               n_accept=np.empty(1, np.int32), lam=np.empty(1), den=np.empty((1, n_alt)), vh=np.empty((1, n_freq)))

    def call(n_tan=3, den0_stride=0, alt_stride=0, basis_stride=0, options=None, prior=None, flags=_native.FLAG_SHARED_FIELD,
             basis=B9, mode=0):
        return ctx.vfo_lm_fit(w["f"].ctypes.data, n_freq, w["den"].ctypes.data, w["bmag"].ctypes.data, w["bpsi"].ctypes.data,
                              w["alt"].ctypes.data, 1, n_alt, den0_stride, alt_stride, mult.ctypes.data, w["n_points"], mode,
                              None if basis is None else basis.ctypes.data, n_tan, basis_stride, obs.ctypes.data, None,
                              None if prior is None else prior.ctypes.data, options, out["c"].ctypes.data,
                              out["cost"].ctypes.data, out["status"].ctypes.data, out["n_eval"].ctypes.data,
                              out["n_accept"].ctypes.data, out["lam"].ctypes.data, out["den"].ctypes.data,
                              out["vh"].ctypes.data, None, None, flags)

    def options(**kw):
        base = dict(max_iter=20, reserved=0, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, step_max=1.0, ftol=1e-10, xtol=1e-10)
        return _native.LmOptions(**dict(base, **kw))

    for kw, text in ((dict(n_tan=0), "n_tan"), (dict(n_tan=9), "n_tan"), (dict(den0_stride=n_alt - 1), "stride"),
                     (dict(alt_stride=1), "stride"), (dict(basis_stride=3 * n_alt - 1), "stride"), (dict(basis=None), "null"),
                     (dict(options=options(max_iter=0)), "max_iter"), (dict(options=options(lambda0=0.0)), "lambda0"),
                     (dict(options=options(lambda_up=1.0)), "lambda_up"), (dict(options=options(xtol=float("nan"))), "xtol"),
                     (dict(prior=np.array([0.0, -1.0, 0.0])), "prior_weight"),
                     (dict(prior=np.array([0.0, float("nan"), 0.0])), "prior_weight"),
                     (dict(prior=np.array([0.0, float("inf"), 0.0])), "prior_weight"), (dict(mode=2), "mode"),
                     (dict(flags=_native.FLAG_ASYNC), "ASYNC"), (dict(flags=0x100), "flag")):
        assert call(**kw) == _native.EINVAL, kw
        assert text in _native.last_error(), (kw, _native.last_error())
    assert call() == _native.OK and out["status"][0] in CONVERGED              # (the same arguments, nothing wrong)
    assert same_bits(out["c"][0, :3], fit_case(w).c[0])


# ---- a column taller than the JVP's plan takes whole (1332 levels): the peak pre-pass, once per evaluation ----

def test_tall_column_waits_once_per_evaluation(arithmetic_cases):
    col, B, f, obs = arithmetic_cases["o"]
    pick = np.round(np.linspace(0, 129, 10)).astype(int)
    f, obs = f[pick], obs[pick]
    extra = 1400 - col["alt"].size                           # 620 -> 1400 levels, all of the new ones above the peak
    step = col["alt"][-1] - col["alt"][-2]
    alt = np.concatenate([col["alt"], col["alt"][-1] + step * np.arange(1, extra + 1)])
    den = np.concatenate([col["den"], col["den"][-1] * np.exp(-np.arange(1, extra + 1) / 50.0)])
    bmag = np.concatenate([col["bmag"], np.full(extra, col["bmag"][-1])])
    bpsi = np.concatenate([col["bpsi"], np.full(extra, col["bpsi"][-1])])
    assert int(np.argmax(den)) == int(np.argmax(col["den"]))
    B_tall = np.concatenate([B, np.zeros((B.shape[0], extra))], axis=1)
    short = fitting.fit_profiles_lm(f, obs[None, :], col["den"], col["bmag"], col["bpsi"], col["alt"], B, col["mode"],
                                    col["n_points"], max_iter=3)
    assert _native.host_context(0).lm_fit_counters() == (3, 13, 1)
    fitting.fit_profiles_lm(f, obs[None, :], den, bmag, bpsi, alt, B_tall, col["mode"], col["n_points"], max_iter=3)
    tall = fitting.fit_profiles_lm(f, obs[None, :], den, bmag, bpsi, alt, B_tall, col["mode"], col["n_points"], max_iter=3)
    assert _native.host_context(0).lm_fit_counters() == (3, 13, 3 + 1)
    # the levels above the peak do not enter the operator or its derivative
    assert np.allclose(tall.c, short.c, rtol=1e-9, atol=0.0) and np.allclose(tall.cost, short.cost, rtol=1e-9)
    assert np.array_equal(tall.status, short.status) and np.allclose(tall.den[0, :col["alt"].size], short.den[0], rtol=1e-12)
