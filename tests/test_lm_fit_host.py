"""Host checks of the Levenberg-Marquardt fit, no GPU: the ABI of prhf_vfo_lm_fit_f64 and the
argument checks of ``fitting.fit_profiles_lm``; the rule's NumPy restatement (tests/lm_rule.py) on a linear model
against ``numpy.linalg.lstsq``; and tests/devtools/lm_step_host.cpp - pyrayhf_amd/csrc/prhf_lm_step.h, the header the
kernel includes, in a stand-alone program built with g++ under ASan + UBSan - against the restatement, bit for bit."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lm_rule
from conftest import REPO
from pyrayhf_amd import _native, fitting


# ---- ABI ----

def test_symbol_header_and_binding_agree():
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    assert re.search(r"\bint\s+prhf_vfo_lm_fit_f64\s*\(", text) and re.search(r"\bint\s+prhf_lm_fit_counters\s*\(", text)
    assert {"prhf_vfo_lm_fit_f64", "prhf_lm_fit_counters"} <= set(_native.exported_symbols())
    lib = _native.load()
    assert hasattr(lib, "prhf_vfo_lm_fit_f64") and hasattr(lib, "prhf_lm_fit_counters")
    # the argument list of the declaration: one binding type per parameter
    decl = re.search(r"\bint\s+prhf_vfo_lm_fit_f64\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == len(lib.prhf_vfo_lm_fit_f64.argtypes) == 32
    # the options struct and the constants
    fields = re.search(r"typedef struct prhf_lm_options \{(.*?)\} prhf_lm_options;", text, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b(?:int32_t|double)\s+(\w+)\s*;", fields)
    assert names == [n for n, _ in _native.LmOptions._fields_]
    assert ctypes.sizeof(_native.LmOptions) == 8 + 6 * 8
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(PRHF_LM_[A-Z_]+)\s+(\d+)\b", text)}
    want = {"PRHF_LM_RUNNING": fitting.LM_RUNNING, "PRHF_LM_CONVERGED_F": fitting.LM_CONVERGED_F,
            "PRHF_LM_CONVERGED_X": fitting.LM_CONVERGED_X, "PRHF_LM_SINGULAR": fitting.LM_SINGULAR,
            "PRHF_LM_NO_DATA": fitting.LM_NO_DATA, "PRHF_LM_NO_COST": fitting.LM_NO_COST,
            "PRHF_LM_MAX_TANGENTS": _native.LM_MAX_TANGENTS, "PRHF_LM_FIT_COUNTERS": _native.LM_FIT_COUNTERS}
    assert defines == want
    assert (lm_rule.RUNNING, lm_rule.CONVERGED_F, lm_rule.CONVERGED_X, lm_rule.SINGULAR, lm_rule.NO_DATA,
            lm_rule.NO_COST) == tuple(want[k] for k in list(want)[:6])
    assert _native.ABI_VERSION == 4


def test_null_context_is_einval_with_a_message():
    lib = _native.load()
    args = [None] * 32
    for i, t in enumerate(lib.prhf_vfo_lm_fit_f64.argtypes):
        if t in (ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32):
            args[i] = 0
    assert lib.prhf_vfo_lm_fit_f64(*args) == _native.EINVAL
    assert "null context" in _native.last_error()
    assert lib.prhf_lm_fit_counters(None, None) == _native.EINVAL


# ---- the wrapper's argument checks: raised before the library is reached ----

def _inputs(n_iono=2, n_alt=12, n_freq=5, n_tan=3):
    rng = np.random.default_rng(5)
    alt = np.linspace(90.0, 300.0, n_alt)
    return dict(freq=np.linspace(2.0, 4.0, n_freq), vh_obs=200.0 + rng.random((n_iono, n_freq)),
                den0=1e11 * (1.0 + rng.random((n_iono, n_alt))), bmag=np.full(n_alt, 4e-5), bpsi=np.full(n_alt, 30.0), alt=alt,
                basis=rng.random((n_tan, n_alt)))


@pytest.mark.parametrize("change, match", [
    (dict(basis=np.zeros((0, 12))), "directions"),
    (dict(basis=np.zeros((9, 12))), "directions"),
    (dict(basis=np.zeros((3, 11))), "basis must be"),
    (dict(basis=np.zeros((3, 3, 12))), "basis must be"),
    (dict(den0=np.ones((3, 12))), "den0 must be"),
    (dict(den0=np.ones((2, 2, 12))), "den0"),
    (dict(vh_obs=np.ones((2, 4))), "vh_obs must be"),
    (dict(bmag=np.ones(11)), "bmag and bpsi"),
    (dict(bpsi=np.ones((3, 12))), "bmag and bpsi"),
    (dict(alt=np.ones((2, 12))), "alt must be"),
    (dict(prior_weight=[1.0, -1.0, 0.0]), "prior_weight"),
    (dict(prior_weight=[1.0, float("nan"), 0.0]), "prior_weight"),
    (dict(prior_weight=[1.0, 1.0]), "prior_weight must be"),
    (dict(c0=np.zeros(2)), "c0 must be"),
    (dict(max_iter=0), "max_iter"),
    (dict(mode="Z"), "mode must be"),
    (dict(prior_weight=[1.0, float("inf"), 0.0]), "prior_weight must be finite"),
])
def test_bad_arguments_raise_before_any_native_call(monkeypatch, change, match):
    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    kw = dict(_inputs(), **change)
    with pytest.raises(ValueError, match=match):
        fitting.fit_profiles_lm(**kw)


def test_minimize_parameters_many_points_to_the_derivative_fit():
    import pyrayhf_amd
    assert "fit_profiles_lm" in pyrayhf_amd.__all__ and "fit_profiles_lm" in fitting.__all__ and "LM_NO_DATA" in fitting.__all__
    assert "fit_profiles_lm" in fitting.minimize_parameters_many.__doc__
    with pytest.raises(NotImplementedError, match="fit_profiles_lm"):
        fitting.minimize_parameters_many([], [], [], [1.0], np.zeros((0, 1)), np.zeros(3), np.zeros(3), np.zeros(3),
                                         method="leastsq")


# ---- the rule on a linear model ----

def _linear_case(seed, n_freq, n_tan, nan_obs=0, nan_model=0, noise=1e-3):
    rng = np.random.default_rng(seed)
    D = rng.normal(size=(n_freq, n_tan)) * 40.0
    vh0 = 250.0 + 30.0 * rng.random(n_freq)
    c_true = rng.uniform(-0.08, 0.08, n_tan)
    obs = vh0 + D @ c_true + noise * rng.normal(size=n_freq)
    if nan_obs:
        obs[rng.choice(n_freq, nan_obs, replace=False)] = np.nan
    if nan_model:
        vh0[rng.choice(n_freq, nan_model, replace=False)] = np.nan
    return obs, vh0, D


def _evaluate(vh0, D):
    def evaluate(c):
        v = vh0.copy()
        for t in range(D.shape[1]):
            v = v + D[:, t] * c[t]
        return v, D
    return evaluate


@pytest.mark.parametrize("n_freq, n_tan, noise, ftol", [(10, 3, 0.0, 1e-10), (70, 8, 0.0, 1e-10), (130, 1, 0.0, 1e-10),
                                                        (64, 4, 0.0, 1e-10), (70, 8, 1e-3, 1e-15), (10, 3, 1e-3, 1e-15)])
def test_linear_model_reaches_the_least_squares_solution(n_freq, n_tan, noise, ftol):
    """The default xtol ends the iteration at a step of 1e-10 relative, by design short of 1e-12 in the coefficients:
    the cases ask for 1e-14.  Likewise, with a residual floor (noise) the default ftol - a relative gain of 1e-10 -
    would end it early; those cases ask for 1e-15."""
    obs, vh0, D = _linear_case(11 + n_freq, n_freq, n_tan, nan_obs=2 if n_freq > 10 else 0, noise=noise)
    got = lm_rule.fit(_evaluate(vh0, D), obs, n_tan, ftol=ftol, xtol=1e-14)
    kept = np.isfinite(obs)
    want = np.linalg.lstsq(D[kept], (obs - vh0)[kept], rcond=None)[0]
    assert got["status"] in (lm_rule.CONVERGED_F, lm_rule.CONVERGED_X), got["status"]
    assert np.max(np.abs(got["c"] - want)) <= 1e-12 * np.max(np.abs(want)), (got["c"], want)
    h = got["history"]
    assert np.all(np.diff(h) <= 0.0) and h[-1] == got["cost"] and got["n_accept"] <= got["n_eval"] <= 20


@pytest.mark.parametrize("n_freq, n_tan", [(10, 3), (70, 8), (130, 1), (64, 4)])
def test_linear_model_with_the_default_tolerances(n_freq, n_tan):
    """What the tabulated defaults reach on the consistent systems above.  CONVERGED_X leaves one step untaken, of at
    most xtol (max|c| + xtol); on a linear model the distance to the solution is (1 + lambda) times that step, lambda
    <= lambda0 after an acceptance: the coefficients are good to 2 xtol = 2e-10 relative, not to 1e-12 (measured:
    2e-12 at worst on these four - the steps shrink by the factor lambda, so the last one is far below the test's limit)."""
    obs, vh0, D = _linear_case(11 + n_freq, n_freq, n_tan, nan_obs=2 if n_freq > 10 else 0, noise=0.0)
    got = lm_rule.fit(_evaluate(vh0, D), obs, n_tan)
    kept = np.isfinite(obs)
    want = np.linalg.lstsq(D[kept], (obs - vh0)[kept], rcond=None)[0]
    rel = np.max(np.abs(got["c"] - want)) / np.max(np.abs(want))
    print(f"defaults, F = {n_freq}, T = {n_tan}: status {got['status']} after {got['n_eval']} evaluations, "
          f"max |c - lstsq| / max |c| = {rel:.2e}")
    assert got["status"] in (lm_rule.CONVERGED_F, lm_rule.CONVERGED_X) and got["n_eval"] <= 20
    assert rel <= 2.0 * lm_rule.DEFAULTS["xtol"]


def test_linear_model_with_a_prior_reaches_the_ridge_solution():
    obs, vh0, D = _linear_case(3, 12, 4)
    w = np.array([0.0, 5.0, 50.0, 500.0])
    got = lm_rule.fit(_evaluate(vh0, D), obs, 4, prior_weight=w, max_iter=40, ftol=1e-15, xtol=1e-14)
    want = np.linalg.solve(D.T @ D + np.diag(w), D.T @ (obs - vh0))
    assert got["status"] in (lm_rule.CONVERGED_F, lm_rule.CONVERGED_X)
    assert np.max(np.abs(got["c"] - want)) <= 1e-12 * np.max(np.abs(want))


def test_no_data_and_no_cost():
    obs, vh0, D = _linear_case(7, 10, 3)
    calls = []

    def evaluate(c):
        calls.append(c)
        return _evaluate(vh0, D)(c)
    got = lm_rule.fit(evaluate, np.full(10, np.nan), 3, c0=[0.01, 0.0, -0.01])
    assert got["status"] == lm_rule.NO_DATA and np.isnan(got["cost"]) and np.isnan(got["vh"]).all()
    assert np.array_equal(got["c"], [0.01, 0.0, -0.01]) and got["n_eval"] == 1 and got["n_accept"] == 0 and len(calls) == 1
    # a model without a single finite height on the kept frequencies: the fill is NaN, and so is the cost
    got = lm_rule.fit(_evaluate(np.full(10, np.nan), D), obs, 3)
    assert got["status"] == lm_rule.NO_COST and not np.isfinite(got["cost"]) and got["n_eval"] == 1
    # a singular normal matrix (a direction nothing depends on, twice) is damped, not refused
    D2 = np.concatenate([D, D[:, :1]], axis=1)
    got = lm_rule.fit(_evaluate(vh0, D2), obs, 4)
    assert got["status"] in (lm_rule.CONVERGED_F, lm_rule.CONVERGED_X)


# ---- the header on a host, under the sanitizers, against the restatement ----

def _pattern(v):
    """The 64 bits of a double; every NaN counts as one value (its sign and payload are the processor's)."""
    v = np.asarray(v, dtype=np.float64)
    return -1 if np.isnan(v) else int(v.view(np.uint64))


def _word(text):
    return _pattern(np.array(int(text, 16), dtype=np.uint64).view(np.float64))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lm_step_host") / "lm_step_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"),
                    os.path.join(REPO, "tests", "devtools", "lm_step_host.cpp"), "-o", str(exe)], check=True)
    return exe


def _header_against_the_restatement(exe, tmp_path, n_freq, n_tan, cases, starts, w, prior, options):
    """Runs lm_step_host on ``cases`` (obs, vh0, D) from ``starts`` and asserts every line of its output - c, c_eval,
    cost, lambda and the status after every evaluation, then the end's status, counts, A, g and delta - equal to
    tests/lm_rule.py's on the same model, bit for bit.  Returns the restatement's ``(result, trace)`` per case."""
    head = [len(cases), n_tan, n_freq, options["max_iter"], options["lambda0"], options["lambda_up"], options["lambda_down"],
            options["step_max"], options["ftol"], options["xtol"], 1.0 if prior else 0.0]
    blob = [np.array(head, dtype=np.float64)]
    for (obs, vh0, D), c0 in zip(cases, starts):
        blob += [obs, vh0, D.ravel(), c0, w]
    path = tmp_path / "cases.bin"
    np.concatenate(blob).astype(np.float64).tofile(path)
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) * (options["max_iter"] + 1)
    out = []
    for q, ((obs, vh0, D), c0) in enumerate(zip(cases, starts)):
        trace = []
        got = lm_rule.fit(_evaluate(vh0, D), obs, n_tan, c0=c0, prior_weight=w if prior else None, trace=trace, **options)
        mine = lines[q * (options["max_iter"] + 1):(q + 1) * (options["max_iter"] + 1)]
        k_done = 0
        for k in range(options["max_iter"]):
            words = mine[k].split()
            if k < len(trace):
                k_done = k
            c, c_eval, cost, lam, status = trace[k_done]                           # (a frozen case repeats its last state)
            want = [_pattern(x) for x in c] + [_pattern(x) for x in c_eval] + [_pattern(cost), _pattern(lam)]
            assert [_word(x) for x in words[:-1]] == want, (q, k)
            assert int(words[-1]) == status, (q, k)
        end = mine[-1].split()
        assert end[0] == "end" and [int(x) for x in end[1:4]] == [got["status"], got["n_eval"], got["n_accept"]], (q, end[:4])
        tail = [_word(x) for x in end[4:]]
        want = [_pattern(x) for x in got["A"].ravel()] + [_pattern(x) for x in got["g"]] + [_pattern(x) for x in got["delta"]]
        assert tail == want, q
        out.append((got, trace))
    return out


@pytest.mark.parametrize("n_freq, n_tan, prior", [(10, 3, False), (70, 8, True), (130, 1, False), (65, 5, True)])
def test_header_on_the_host_equals_the_restatement_bit_for_bit(tmp_path, host_program, n_freq, n_tan, prior):
    options = dict(lm_rule.DEFAULTS, max_iter=12)
    rng = np.random.default_rng(n_freq)
    cases = [_linear_case(100 + q, n_freq, n_tan, nan_obs=(q % 3) * min(3, n_freq // 4), nan_model=(q % 2) * 2) for q in range(4)]
    cases.append((np.full(n_freq, np.nan),) + cases[0][1:])                       # NO_DATA
    cases.append((cases[0][0], np.full(n_freq, np.nan), cases[0][2]))             # NO_COST
    starts = [rng.uniform(-0.05, 0.05, n_tan) if q % 2 else np.zeros(n_tan) for q in range(len(cases))]
    w = rng.uniform(0.0, 10.0, n_tan)
    fits = _header_against_the_restatement(host_program, tmp_path, n_freq, n_tan, cases, starts, w, prior, options)
    seen = {got["status"] for got, _ in fits}
    assert lm_rule.NO_DATA in seen and lm_rule.NO_COST in seen and seen & {lm_rule.CONVERGED_F, lm_rule.CONVERGED_X}


# ---- the rule's rare ends: SINGULAR with its retries, both clamps of lambda, the step cap, the fill's floor ----

RARE_F = 70


@pytest.mark.parametrize("n_tan", [2, 5, 8])
def test_header_on_the_host_equals_the_restatement_at_the_rare_ends(tmp_path_factory, host_program, n_tan):
    """Four option sets on the linear model (F = 70, seed 1, noise 1e-3), each one run of the sanitized program and each
    line of it the restatement's, bit for bit; what the rule must do there is asserted on the restatement's side.
    1. D x 2^520 from c0 = 0: the rows and the cost are finite, D^T D overflows, the first column of the factor is
       inf / inf: no pivot is positive at any lambda, eight retries, SINGULAR with lambda0 lambda_up^8 - 1e5 with the
       defaults, the upper clamp 1e12 from lambda0 = 1e8.  The same run has NO_DATA, NO_COST, and heights of 50 - 80 km
       with two modelled NaN, where the fill is its floor of 100 km and not the mean.
    2. ftol = xtol = 0, lambda_up = 1e3, lambda_down = 1e6, 40 evaluations: accepted steps take lambda to the lower
       clamp, then the cost stops falling at its rounding floor and the rejections take it to the upper one; nothing ends it.
    3. step_max = 0.01: the first steps are scaled to the cap, and the fit still converges."""
    obs, vh0, D = _linear_case(1, RARE_F, n_tan, noise=1e-3)
    zeros, w = np.zeros(n_tan), np.zeros(n_tan)
    huge = (obs, vh0, D * 2.0 ** 520)
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.isfinite(huge[2]).all() and np.isinf(np.diag(huge[2].T @ huge[2])).all()
    low_obs, low_vh0, low_D = _linear_case(2, RARE_F, n_tan, nan_model=2)
    low = (low_obs - 200.0, low_vh0 - 200.0, low_D)
    assert np.nanmax(low[1]) < 100.0 and np.isnan(low[1]).sum() == 2 and np.isfinite(low[0]).all()
    seen = set()

    def run(name, cases, **options):
        options = dict(lm_rule.DEFAULTS, **options)
        fits = _header_against_the_restatement(host_program, tmp_path_factory.mktemp(name), RARE_F, n_tan, cases,
                                               [zeros] * len(cases), w, False, options)
        seen.update(got["status"] for got, _ in fits)
        return fits

    # 1. SINGULAR
    cases = [huge, (np.full(RARE_F, np.nan), vh0, D), (obs, np.full(RARE_F, np.nan), D), low, (obs, vh0, D)]
    for lambda0, lam_end in ((lm_rule.DEFAULTS["lambda0"], 1e5), (1e8, 1e12)):
        with np.errstate(over="ignore", invalid="ignore"):             # (the overflow is the case)
            fits = run("singular", cases, max_iter=12, lambda0=lambda0)
        got = fits[0][0]
        assert (got["status"], got["n_eval"], got["n_accept"]) == (lm_rule.SINGULAR, 1, 1)
        want = lambda0
        for _ in range(lm_rule.RETRIES):
            want = lm_rule.clamp(want * 10.0)
        assert got["lam"] == want and abs(want - lam_end) <= 4 * np.spacing(lam_end)
        assert np.array_equal(got["delta"], zeros) and np.isfinite(got["cost"]) and np.isinf(got["A"]).any()
        assert [f[0]["status"] for f in fits[1:3]] == [lm_rule.NO_DATA, lm_rule.NO_COST]
    # 2. the rounding floor
    (got, trace), = run("floor", [(obs, vh0, D)], ftol=0.0, xtol=0.0, lambda_up=1e3, lambda_down=1e6, max_iter=40)
    lams = {t[3] for t in trace}
    assert lm_rule.LAMBDA_MIN in lams and lm_rule.LAMBDA_MAX in lams, sorted(lams)
    assert got["status"] == lm_rule.RUNNING and got["n_eval"] == 40 and np.all(np.diff(got["history"]) <= 0.0)
    # 3. the step cap
    (got, trace), = run("cap", [(obs, vh0, D)], step_max=0.01)
    assert lm_rule.capped_run(trace, 0.01) >= 3, [float(np.max(np.abs(t[1] - t[0]))) for t in trace]
    assert got["status"] in (lm_rule.CONVERGED_F, lm_rule.CONVERGED_X) and got["n_eval"] <= lm_rule.DEFAULTS["max_iter"]
    # 4. every end of the rule has been through the header
    assert seen >= {lm_rule.RUNNING, lm_rule.SINGULAR, lm_rule.NO_DATA, lm_rule.NO_COST}
    assert seen & {lm_rule.CONVERGED_F, lm_rule.CONVERGED_X}
