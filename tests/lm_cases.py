"""Columns, bases and drivers that the GPU tests of the Levenberg-Marquardt fit share (tests/test_gpu_lm_fit.py,
tests/test_gpu_lm_fit_edges.py): a helper, not a test.

Columns of fixture g26: the 78-level g (O mode), h and d (X mode), the 620-level o.  Basis: Gaussian bumps of width 0.2
in the normalised bottomside height z = (alt - alt[0]) / (hmF2 - alt[0]).  Observations come from the CPU oracle
(oracle/vfo_numpy.py), never from the code under test."""

import numpy as np

import lm_rule
from conftest import load_golden, same_bits
from oracle import vfo_numpy as orc
from pyrayhf_amd import _native, fitting, library

G26 = load_golden("g26_jacobian.npz")
U = 2.0 ** -52
CENTRES3 = (0.25, 0.575, 0.9)
FIELDS = ("c", "cost", "status", "n_eval", "n_accept", "lam", "den", "vh", "state", "cost_history")


def column(name):
    c = {k: G26[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt")}
    c["mode"], c["n_points"] = str(G26[f"{name}_mode"]), int(G26[f"{name}_n_points"])
    return c


def gauss_basis(alt, den, centres, width=0.2):
    k = int(np.argmax(den))
    z = (alt - alt[0]) / (alt[k] - alt[0])
    return np.exp(-0.5 * ((z[None, :] - np.asarray(centres, dtype=np.float64)[:, None]) / width) ** 2)


def centres_of(n_tan):
    """T centres over the bottomside; one direction sits in its middle."""
    return np.array([0.575]) if n_tan == 1 else np.linspace(0.1, 0.95, n_tan)


def oracle(freq, den, col, mode=None, n_points=None):
    den = np.atleast_2d(den)
    rows = den.shape[0]
    return orc.virtual_heights_batch(freq, den, np.broadcast_to(col["bmag"], (rows, col["bmag"].size)),
                                     np.broadcast_to(col["bpsi"], (rows, col["bpsi"].size)), col["alt"],
                                     mode or col["mode"], n_points or col["n_points"])


def well_posed(name, lo, hi, seed, centres=CENTRES3, max_gap=25.0):
    """Column ``name`` with 10 frequencies on ``lo`` ... ``hi`` x the fixture's highest, a truth of |c_t| <= 0.08 and the
    oracle's trace of it, screened: every frequency reflects for the start and for the truth, and (``max_gap``, km, or
    None) the two traces are that close.  A case that fails the screen is an error of the file that asks for it."""
    col = column(name)
    f = np.linspace(lo, hi, 10) * col["freq"].max()
    B = gauss_basis(col["alt"], col["den"], centres)
    c_true = np.random.default_rng(seed).uniform(-0.08, 0.08, B.shape[0])
    vh_start = oracle(f, col["den"], col)[0]
    obs = oracle(f, col["den"] * np.exp(c_true @ B), col)[0]
    # the screen
    assert np.isfinite(vh_start).all() and np.isfinite(obs).all(), name
    if max_gap is not None:
        assert np.max(np.abs(vh_start - obs)) <= max_gap, (name, float(np.max(np.abs(vh_start - obs))))
    return dict(col, name=name, f=f, B=B, c_true=c_true, obs=obs)


def fit_case(w, **kw):
    return fitting.fit_profiles_lm(w["f"], w["obs"][None, :], w["den"], w["bmag"], w["bpsi"], w["alt"], w["B"], w["mode"],
                                   w["n_points"], **kw)


def device_evaluate(w, one_tangent_at_a_time=False):
    """evaluate(c) of tests/lm_rule.py with the device's own bits: the trial column is lm_synth_kernel's (a fit of one
    evaluation from c returns it), its tangents are one product each, and the rows of ``library.vertical_jvp`` depend
    on their own column and tangent only.  ``one_tangent_at_a_time``: T calls of one tangent each, so that nothing of
    the result went through the JVP's chunking of several tangents."""
    def evaluate(c):
        den = fit_case(w, c0=c, max_iter=1).den[0]
        args = (w["f"], den, w["bmag"], w["bpsi"], w["alt"])
        if not one_tangent_at_a_time:
            return library.vertical_jvp(*args, den[None, :] * w["B"], w["mode"], w["n_points"])
        pairs = [library.vertical_jvp(*args, den * b, w["mode"], w["n_points"]) for b in w["B"]]
        assert all(same_bits(vh, pairs[0][0]) for vh, _ in pairs)
        return pairs[0][0], np.stack([d for _, d in pairs], axis=1)
    return evaluate


def lm_options(**options):
    """``(the options of tests/lm_rule.py, the same as a native LmOptions)``: the defaults with ``options`` over them."""
    o = dict(lm_rule.DEFAULTS, **options)
    return o, _native.LmOptions(int(o["max_iter"]), 0, o["lambda0"], o["lambda_up"], o["lambda_down"], o["step_max"], o["ftol"],
                                o["xtol"])


def native_fit(f, obs, den0, bmag, bpsi, alt, basis, mode, n_points, *, c0=None, prior=None, n_alt=None, n_tan=None,
               den0_stride=None, alt_stride=0, basis_stride=None, **options):
    """prhf_vfo_lm_fit_f64 itself, with a full LmOptions (``lambda_up`` and ``lambda_down`` too) and the ABI's strides:
    an ``LmFit`` with history and state.  ``f`` ascending, ``obs`` (I, F).  NumPy arrays go the host route; with a
    GPU-resident torch ``den0`` every array is a tensor and the call takes device pointers.  ``den0`` one column or I
    rows, ``basis`` (T, N_alt) or (I, T, N_alt), ``bmag`` and ``bpsi`` one row or I packed rows; a stride given here
    overrides the packed one, the array then is the buffer the rows lie in (``n_alt``, ``n_tan``: the shape it hides)."""
    on_gpu = library._is_torch(den0)
    n_iono, n_freq = obs.shape
    n_alt = int(alt.shape[-1]) if n_alt is None else n_alt
    n_tan = int(basis.shape[-2]) if n_tan is None else n_tan
    if den0_stride is None:
        den0_stride = n_alt if den0.ndim == 2 else 0
    if basis_stride is None:
        basis_stride = n_tan * n_alt if basis.ndim == 3 else 0
    _, opt = lm_options(**options)
    flags = _native.FLAG_SHARED_FIELD if bmag.ndim == 1 else 0
    if on_gpu:
        import torch
        dev = den0.device
        ctx = _native.context(dev.index)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        mult, grid_flag = library._device_grid((int(n_points),), dev)
        flags |= _native.FLAG_DEVICE_PTRS | grid_flag
        ptr = lambda x: None if x is None else x.data_ptr()                        # noqa: E731
        new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        int32 = torch.int32
        assert all(x is None or (x.is_contiguous() and x.dtype == torch.float64 and x.device == dev)
                   for x in (f, obs, den0, bmag, bpsi, alt, basis, c0, prior))
    else:
        ctx = _native.host_context(0)
        mult = library._multiplier(n_points)
        ptr = lambda x: None if x is None else x.ctypes.data                       # noqa: E731
        new = lambda *shape, dtype=np.float64: np.empty(shape, dtype=dtype)        # noqa: E731
        int32 = np.int32
        assert all(x is None or (x.flags.c_contiguous and x.dtype == np.float64) for x in (f, obs, den0, bmag, bpsi, alt, basis,
                                                                                           c0, prior))
    ctx.set_math(library.MATH_AUTO)
    c, cost, lam, den, vh = new(n_iono, n_tan), new(n_iono), new(n_iono), new(n_iono, n_alt), new(n_iono, n_freq)
    status, n_eval, n_accept = (new(n_iono, dtype=int32) for _ in range(3))
    history, state = new(n_iono, opt.max_iter), new(n_iono, n_tan * n_tan + 2 * n_tan)
    _native.raise_for(ctx.vfo_lm_fit(
        ptr(f), n_freq, ptr(den0), ptr(bmag), ptr(bpsi), ptr(alt), n_iono, n_alt, den0_stride, alt_stride, ptr(mult),
        int(n_points), fitting._mode_code(mode), ptr(basis), n_tan, basis_stride, ptr(obs), ptr(c0), ptr(prior), opt, ptr(c),
        ptr(cost), ptr(status), ptr(n_eval), ptr(n_accept), ptr(lam), ptr(den), ptr(vh), ptr(history), ptr(state), flags))
    return fitting.LmFit(c, cost, status, n_eval, n_accept, lam, den, vh, history, state)


def native_fit_case(w, obs=None, **kw):
    """``native_fit`` of one ionogram on the case ``w`` (the host route)."""
    obs = w["obs"] if obs is None else obs
    return native_fit(w["f"], np.ascontiguousarray(obs[None, :]), w["den"], w["bmag"], w["bpsi"], w["alt"], w["B"], w["mode"],
                      w["n_points"], **kw)


def state_of(r, i, n_tan):
    """``(A (T, T), g, delta)`` of ionogram ``i`` from the fit's ``state``."""
    s = np.asarray(r.state[i])
    return s[:n_tan * n_tan].reshape(n_tan, n_tan), s[n_tan * n_tan:n_tan * n_tan + n_tan], s[n_tan * n_tan + n_tan:]


def assert_the_rules_state(r, i, want, tag=None):
    """Ionogram ``i`` of the fit ``r`` (with history and state) is tests/lm_rule.py's result ``want``, bit for bit:
    c, cost, lam, status, n_eval, n_accept, vh, cost_history, and A, g and delta from the state."""
    n_tan = want["c"].size
    A, g, delta = state_of(r, i, n_tan)
    assert (int(r.status[i]), int(r.n_eval[i]), int(r.n_accept[i])) == (want["status"], want["n_eval"], want["n_accept"]), tag
    assert same_bits(r.c[i], want["c"]), (tag, "c")
    assert same_bits(r.cost[i], want["cost"]), (tag, "cost", float(r.cost[i]), want["cost"])
    assert same_bits(r.lam[i], want["lam"]), (tag, "lam", float(r.lam[i]), want["lam"])
    assert same_bits(r.cost_history[i], want["history"]), (tag, "cost_history")
    assert same_bits(r.vh[i], want["vh"]), (tag, "vh")
    assert same_bits(A, want["A"]), (tag, "A")
    assert same_bits(g, want["g"]), (tag, "g")
    assert same_bits(delta, want["delta"]), (tag, "delta")
