"""The three derivative entry points (vertical_jacobian, vertical_vjp, vertical_jvp) where fixture
g26 does not reach: tall columns (two and one frequency waves, tangent chunks of 4, 2 and 1, the peak pre-pass, a batch
staged for the higher of two peaks), long grids (2000 and 20 000 points) and bad data (NaN psi, |B|, density, altitude;
negative density; a peak at level 0) - against the 50-digit truth of fixture g28 (tools/gen_g28_derivative_regimes.py).

Bounds: those of tests/test_gpu_jacobian.py, test_gpu_jvp.py and test_gpu_vjp.py - 4 x e_ref[mode] of fixture g26 per
Jacobian row and unit-tangent column, 4 e_ref max|J_mp| ||t||_1 for a dense tangent, the reordering bound
n_freq 2^-52 sum|g J| for the VJP against the Jacobian's rows, 8 e_ref sum|g| max|J_mp| ||t||_1 for the adjoint identity.
The four cases on which the float64 restatement itself is farther than g26's e_ref from the truth (t3b, t4a, t4b,
lo2k620: the fixture's ``own_e_ref``) take their own recorded e_ref in its place.  The measured ratios go to
profiles/jacobian_parity.md with each case's launch regime."""

import numpy as np
import pytest

import derivative_regimes as dr
from conftest import load_golden, same_bits
from oracle import vfo_numpy as orc
from parity_report import put_section
from pyrayhf_amd import library

pytestmark = pytest.mark.gpu

HEADING = "# Derivative kernels on tall columns, long grids and bad data (fixture g28)"


@pytest.fixture(scope="module")
def g28():
    return load_golden("g28_derivative_regimes.npz")


@pytest.fixture(scope="module")
def e_ref(g28):
    g26 = load_golden("g26_jacobian.npz")
    base = {"O": float(g26["e_ref_O"]), "X": float(g26["e_ref_X"])}
    own = {str(n) for n in g28["own_e_ref"]}
    out = {str(n): (float(g28[f"{n}_e_ref"]) if str(n) in own else base[str(g28[f"{n}_mode"])]) for n in g28["cases"]}
    assert own == {"t3b", "t4a", "t4b", "lo2k620"} and all(out[n] <= 2.5 * base[str(g28[f"{n}_mode"])] for n in own)
    return out, own


class Case:
    """One fixture case in batch form: den, bmag, bpsi (P, n_alt); alt as stored; vh_mp (P, F); jac_mp (P, F, peak)."""

    def __init__(self, g, name):
        self.name, self.kind = name, dr.kind_of(g, name)
        self.mode, self.n_points = str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])
        self.freq, self.alt = g[f"{name}_freq"], g[f"{name}_alt"]
        self.den, self.bmag, self.bpsi = (np.atleast_2d(g[f"{name}_{k}"]) for k in ("den", "bmag", "bpsi"))
        self.vh_mp = np.atleast_2d(g[f"{name}_vh_mp"])
        self.jac_mp = g[f"{name}_jac_mp"].reshape(self.den.shape[0], self.freq.size, -1)
        self.regime = g[f"{name}_regime"].tolist()
        self.P, self.n_alt = self.den.shape
        self.F, self.peak = self.freq.size, self.jac_mp.shape[-1]
        self.K = [int(np.argmax(d)) for d in self.den]
        self.args = (self.freq, self.den, self.bmag, self.bpsi, self.alt)
        self.tail = (self.mode, self.n_points)

    def levels(self):
        """(P, T) levels of the unit tangents: every level below the peak, or - tall - 24 of them: 0, K - 1, and jm, j,
        j + 1 of every frequency's reflection bracket, filled up with a regular stride."""
        if self.kind != "tall":
            assert self.P == 1
            return np.arange(self.K[0])[None, :]
        out = []
        for p in range(self.P):
            K, f_hz = self.K[p], self.freq * 1e6
            pick = {0, K - 1}
            for f in f_hz:
                c = orc.ratio_X(self.den[p, :K], f) + (orc.ratio_Y(f, self.bmag[p, :K]) if self.mode == "X" else 0.0)
                r = np.maximum.accumulate(c)
                if r[-1] >= 1.0 and not r[0] > 1.0:
                    j = int(np.nonzero(r <= 1.0)[0][-1])
                    pick |= {int(np.argmax(c[: j + 1])), j, min(j + 1, K - 1)}
            assert len(pick) <= dr.N_UNIT
            for k in np.linspace(0, K - 1, 64).astype(int):
                if len(pick) < dr.N_UNIT:
                    pick.add(int(k))
            out.append(sorted(pick))
        return np.array(out)

    def dense(self):
        """(P, 3, n_alt): den * u, u uniform in (-1, 1) (a NaN density - at or above the bottomside's end - stays NaN)"""
        u = np.random.default_rng(28).uniform(-1.0, 1.0, size=(self.P, 3, self.n_alt))
        return self.den[:, None, :] * u

    def upstream(self, vh):
        g = np.random.default_rng(128).uniform(-2.0, 2.0, size=(self.P, self.F))
        g[~np.isfinite(vh)] = 0.0
        return g


@pytest.fixture(scope="module")
def cases(g28):
    return [Case(g28, str(n)) for n in g28["cases"]]


@pytest.fixture(scope="module")
def computed(cases):
    """name -> dict of the three entry points' results, computed once."""
    out = {}
    for c in cases:
        vh, J = library.vertical_jacobian(*c.args, *c.tail)
        lev = c.levels()
        units = np.zeros((c.P, lev.shape[1], c.n_alt))
        for p in range(c.P):
            units[p, np.arange(lev.shape[1]), lev[p]] = 1.0
        vh_u, cols = library.vertical_jvp(*c.args, units, *c.tail)
        vh_d, dense = library.vertical_jvp(*c.args, c.dense(), *c.tail)
        g = c.upstream(vh)
        back = library.vertical_vjp(*c.args, g, *c.tail)
        out[c.name] = {"vh": vh, "J": J, "lev": lev, "cols": cols, "dense": dense, "g": g, "vjp": back, "vh_u": vh_u, "vh_d": vh_d}
    return out


# ---- a. every row against the truth ------------------------------------------------------------------------------------
def test_every_row_of_g28_against_the_truth(cases, computed, e_ref):
    lines = [HEADING, "",
             "Regime: frequency waves / staged levels of the VJP and of the Jacobian launch, tangents per launch / staged levels "
             "of the JVP's unit tangents (24 on the tall cases, every level below the peak elsewhere) and, in brackets, tangents "
             "per launch of its three dense tangents, as the planning tools give them.  J and JVP: worst row err = max_k |. - J_mp| / max_k |J_mp| over e_ref (bound 4; e_ref is g26's per "
             "mode, the case's own where marked *).  dense: |dvh - J_mp t| over 4 e_ref max|J_mp| ||t||_1.  VJP: "
             "|vjp - sum_f g J| over n_freq 2^-52 sum_f |g J|.  adjoint: |<g, J t> - <J^T g, t>| over "
             "8 e_ref sum|g| max|J_mp| ||t||_1.  Bounds: 1 for the last three.  Written by tests/test_gpu_derivative_regimes.py.", "",
             "| case | mode | n_points | levels | peak | VJP | Jacobian | JVP | e_ref | J / e_ref | JVP / e_ref | dense | VJP | adjoint |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    failures = []
    e_ref, own_names = e_ref
    for c in cases:
        r, e = computed[c.name], e_ref[c.name]
        assert r["J"].shape == (c.P, c.F, c.n_alt) and r["vjp"].shape == (c.P, c.n_alt), c.name
        assert np.array_equal(np.isnan(r["vh"]), np.isnan(c.vh_mp)), (c.name, r["vh"], c.vh_mp)
        scale = np.abs(c.jac_mp).max(axis=2)                                                  # (P, F)
        live = scale > 0
        assert np.array_equal(live, np.isfinite(c.vh_mp)), c.name
        safe = np.where(live, scale, 1.0)
        err_j = np.where(live, np.abs(r["J"][:, :, :c.peak] - c.jac_mp).max(axis=2) / safe, 0.0)
        truth_cols = np.stack([c.jac_mp[p][:, r["lev"][p]] for p in range(c.P)])              # (P, F, T)
        err_u = np.where(live, np.abs(r["cols"] - truth_cols).max(axis=2) / safe, 0.0)
        t = c.dense()
        tk = np.nan_to_num(t[:, :, :c.peak])                                                  # (levels at or above a profile's K: zero columns of J_mp)
        for p in range(c.P):
            tk[p, :, c.K[p]:] = 0.0
        want = np.einsum("pfk,ptk->pft", c.jac_mp.astype(np.longdouble), tk.astype(np.longdouble))
        norm1 = np.abs(tk).sum(axis=2)                                                        # (P, 3)
        bound_d = 4.0 * e * scale[:, :, None] * norm1[:, None, :]
        diff_d = np.abs(r["dense"].astype(np.longdouble) - want).astype(np.float64)
        ratio_d = float(np.where(bound_d > 0, diff_d / np.where(bound_d > 0, bound_d, 1.0), 0.0).max())
        assert not r["dense"][~live].any() and not r["cols"][~live].any(), c.name
        terms = np.where(live[:, :, None], r["g"][:, :, None].astype(np.longdouble) * r["J"].astype(np.longdouble), 0.0)
        bound_v = c.F * 2.0 ** -52 * np.abs(terms).sum(axis=1).astype(np.float64)
        diff_v = np.abs(r["vjp"].astype(np.longdouble) - terms.sum(axis=1)).astype(np.float64)
        ratio_v = float(np.where(bound_v > 0, diff_v / np.where(bound_v > 0, bound_v, 1.0), 0.0).max())
        lhs = (r["g"].astype(np.longdouble)[:, :, None] * r["dense"].astype(np.longdouble)).sum(axis=1)          # (P, 3)
        rhs = np.einsum("ptk,pk->pt", tk.astype(np.longdouble), r["vjp"][:, :c.peak].astype(np.longdouble))
        bound_a = 8.0 * e * (np.abs(r["g"]) * scale).sum(axis=1)[:, None] * norm1
        ratio_a = float(np.where(bound_a > 0, np.abs(lhs - rhs).astype(np.float64) / np.where(bound_a > 0, bound_a, 1.0), 0.0).max())
        own = "*" if c.name in own_names else ""
        reg = c.regime
        lines.append(f"| {c.name} | {c.mode} | {c.n_points} | {c.n_alt} | {c.peak} | {reg[0]} / {reg[1]} | {reg[2]} / {reg[3]} | "
                     f"{reg[4]} / {reg[5]} ({reg[6]}) | {e:.3e}{own} | {err_j.max() / e:.2f} | {err_u.max() / e:.2f} | {ratio_d:.3f} | "
                     f"{ratio_v:.3f} | {ratio_a:.3e} |")
        print(lines[-1])
        if not (err_j <= 4.0 * e).all():
            failures.append((c.name, "jacobian", float(err_j.max() / e)))
        if not (err_u <= 4.0 * e).all():
            failures.append((c.name, "jvp unit tangents", float(err_u.max() / e)))
        if not ((diff_d <= bound_d).all() and np.isfinite(r["dense"]).all()):
            failures.append((c.name, "jvp dense tangents", ratio_d))
        if not (diff_v <= bound_v).all():
            failures.append((c.name, "vjp against the jacobian rows", ratio_v))
        if not ratio_a <= 1.0:
            failures.append((c.name, "adjoint identity", ratio_a))
        if not (diff_v[bound_v == 0] == 0).all():
            failures.append((c.name, "vjp non-zero where every term is zero", 0.0))
    put_section(lines)
    assert not failures, failures


# ---- b. conventions on every case ----------------------------------------------------------------------------------------
def test_conventions_on_every_case(cases, computed):
    without = 0
    for c in cases:
        r = computed[c.name]
        vh = r["vh"]
        dead = np.isnan(vh)
        without += int(dead.sum())
        for key in ("J", "vjp", "cols", "dense"):
            assert np.isfinite(r[key]).all(), (c.name, key)
        assert not r["J"][dead].any() and r["J"][~dead].any(axis=1).all(), c.name            # zero exactly where vh is NaN
        assert not r["cols"][dead].any() and not r["dense"][dead].any(), c.name
        for p in range(c.P):
            assert not r["J"][p, :, c.K[p]:].any() and not r["vjp"][p, c.K[p]:].any(), (c.name, p)
            if dead[p].all():
                assert not r["vjp"][p].any(), c.name
        want = np.atleast_2d(library.vertical_forward_operator(*c.args, *c.tail))
        assert same_bits(vh, want) and same_bits(r["vh_u"], want) and same_bits(r["vh_d"], want), c.name
        # a NaN upstream gradient at a pair without a value, NaN tangent entries at and above the peak: no bit changes
        g = r["g"].copy()
        g[dead] = np.nan
        assert same_bits(library.vertical_vjp(*c.args, g, *c.tail), r["vjp"]), c.name
        t = c.dense()
        for p in range(c.P):
            t[p, :, c.K[p]:] = np.nan
        vh2, got = library.vertical_jvp(*c.args, t, *c.tail)
        assert same_bits(got, r["dense"]) and same_bits(vh2, vh), c.name
        if dead.all():                                 # no pair has a value: not one tangent entry matters
            _, got = library.vertical_jvp(*c.args, np.full_like(t, np.nan), *c.tail)
            assert not got.any() and np.isfinite(got).all(), c.name
    assert without >= 60


# ---- c. NaN that must not matter, NaN that takes everything --------------------------------------------------------------
def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _three(args, g, t, mode, n_points):
    """(vh, J, vjp, dvh) of the three entry points as host arrays."""
    vh, J = (_host(x) for x in library.vertical_jacobian(*args, mode, n_points))
    vjp = _host(library.vertical_vjp(*args, g, mode, n_points))
    vh2, dvh = (_host(x) for x in library.vertical_jvp(*args, t, mode, n_points))
    assert same_bits(vh, vh2)
    return vh, J, vjp, dvh


@pytest.fixture(scope="module")
def column(g28):
    """The clean 78-level column (g26's case h), an upstream gradient and two tangents."""
    c = {k: g28[f"lx2k_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt")}
    rng = np.random.default_rng(3)
    return c, rng.uniform(-2.0, 2.0, size=c["freq"].size), c["den"][None, :] * rng.uniform(-1.0, 1.0, size=(2, c["den"].size))


@pytest.mark.parametrize("mode,n_points", [("O", 65), ("X", 64)])
def test_a_nan_above_the_peak_changes_no_bit_and_a_nan_altitude_takes_every_pair(column, mode, n_points):
    c, g, t = column
    K = int(np.argmax(c["den"]))
    clean = _three((c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"]), g, t, mode, n_points)
    assert np.isfinite(clean[0]).any() and clean[1].any()
    for key in ("bmag", "bpsi"):
        d = {k: v.copy() for k, v in c.items()}
        d[key][K + 3] = np.nan
        got = _three((d["freq"], d["den"], d["bmag"], d["bpsi"], d["alt"]), g, t, mode, n_points)
        assert all(same_bits(a, b) for a, b in zip(got, clean)), key
    for level in (K // 2, K + 3):
        alt = c["alt"].copy()
        alt[level] = np.nan
        g_nan = np.full_like(g, np.nan)                # (not read: no pair has a value)
        vh, J, vjp, dvh = _three((c["freq"], c["den"], c["bmag"], c["bpsi"], alt), g_nan, t, mode, n_points)
        assert np.isnan(vh).all() and same_bits(vh, library.vertical_forward_operator(c["freq"], c["den"], c["bmag"], c["bpsi"],
                                                                                      alt, mode, n_points)), level
        for a in (J, vjp, dvh):
            assert np.isfinite(a).all() and not a.any(), level
    again = _three((c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"]), g, t, mode, n_points)
    assert all(same_bits(a, b) for a, b in zip(again, clean))


# ---- d. errors -----------------------------------------------------------------------------------------------------------
def _outcome(call):
    try:
        return ("value", call())
    except Exception as exc:                           # noqa: BLE001 - the type and the message are what is compared
        return ("raise", type(exc), str(exc))


def _same_outcome(got, want, what):
    assert got[0] == want[0], (what, got, want)
    if want[0] == "raise":
        assert got[1] is want[1] and got[2] == want[2], (what, got, want)


@pytest.mark.parametrize("resident", ["numpy", "torch"])
@pytest.mark.parametrize("defect", ["negative density", "peak at level 0"])
@pytest.mark.parametrize("mode", ["O", "X"])
def test_data_errors_are_the_operators_own(column, mode, defect, resident):
    """Each entry point does what vertical_forward_operator does on the same column - the same exception type and
    message, or the same virtual heights with the derivative's conventions - vertical_vjp, which runs no operator launch,
    included; and the next call on the clean column gives the clean bits."""
    c, g, t = column
    K = int(np.argmax(c["den"]))
    den = c["den"].copy()
    if defect == "negative density":
        den[K // 2] = -den[K // 2]
    else:
        den[0] = 2.0 * den.max()
    if resident == "torch":
        import torch
        put = lambda x: torch.as_tensor(x, device="cuda")          # noqa: E731
    else:
        put = lambda x: x                                          # noqa: E731
    get = _host
    clean_args = tuple(put(c[k]) for k in ("freq", "den", "bmag", "bpsi", "alt"))
    bad_args = (clean_args[0], put(den), *clean_args[2:])
    clean = _three(clean_args, put(g), put(t), mode, 64)
    want = _outcome(lambda: get(library.vertical_forward_operator(*bad_args, mode, 64)))
    jac = _outcome(lambda: [get(x) for x in library.vertical_jacobian(*bad_args, mode, 64)])
    vjp = _outcome(lambda: get(library.vertical_vjp(*bad_args, put(g), mode, 64)))
    jvp = _outcome(lambda: [get(x) for x in library.vertical_jvp(*bad_args, put(t), mode, 64)])
    for got, what in ((jac, "jacobian"), (vjp, "vjp"), (jvp, "jvp")):
        _same_outcome(got, want, (what, defect, mode, resident))
    if want[0] == "value":
        vh = want[1]
        assert same_bits(jac[1][0], vh) and same_bits(jvp[1][0], vh)
        dead = np.isnan(vh)
        assert np.isfinite(jac[1][1]).all() and not jac[1][1][dead].any() and jac[1][1][~dead].any(axis=1).all()
        assert np.isfinite(jvp[1][1]).all() and not jvp[1][1][dead].any()
        assert np.isfinite(vjp[1]).all() and (vjp[1].any() or dead.all())
    again = _three(clean_args, put(g), put(t), mode, 64)
    assert all(same_bits(a, b) for a, b in zip(again, clean))


# ---- e. company ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t5a", "t5b"])
def test_the_two_profiles_of_t5_alone_and_together(g28, computed, name):
    """vh, every Jacobian row and every JVP column (24 unit tangents, 3 dense ones) of a profile have the same bits alone
    and in the batch, although the staging (301 against 1201 levels for the low profile), the waves and the chunks (8
    against 2) differ.  The VJP has them where the launch adds its frequencies on the same number of waves - the high
    profile: one wave alone and together.  The low profile alone runs on four waves, in the batch on one
    (``regime_alone`` of the fixture, read from the planning tools): the same 8 or 10 products g_f J[f, k] - J bit-equal,
    just shown - are added in another order (prhf_plan.h, plan_vjp), so the two results are held to the distance two
    orders of one sum can have, n_freq 2^-52 sum_f |g_f J[f, k]|, not to equal bits.  With the fixture's frequencies the
    low profile has three or four pairs with a value and rows that seldom meet at a level (64 grid points on 300 levels),
    and the two orders happen to round alike; a sweep of twelve frequencies that all reflect in it shows the dependence
    (measured on an MI355X: 23 of the 300 entries differ in t5a, by at most 0.081 of the bound; 14 in t5b, 0.070).  Should the VJP's order ever stop depending on the wave count, the last assertion
    fails: make the bound bit equality then, and take the exception out of include/prhf.h and vertical_vjp's docstring."""
    c, r = Case(g28, name), computed[name]
    t = c.dense()
    alone_regime = g28[f"{name}_regime_alone"]
    assert (np.isfinite(r["vh"]).sum(axis=1) >= 2).all() and np.abs(r["g"]).sum(axis=1).all()
    reordered = 0
    for p in range(c.P):
        one = (c.freq, c.den[p], c.bmag[p], c.bpsi[p], c.alt[p])
        units = np.zeros((r["lev"].shape[1], c.n_alt))
        units[np.arange(r["lev"].shape[1]), r["lev"][p]] = 1.0
        vh, J, vjp, dvh = _three(one, r["g"][p], t[p], *c.tail)
        assert J.any() and vjp.any() and dvh.any(), (name, p)
        assert same_bits(vh, r["vh"][p]) and same_bits(J, r["J"][p]), (name, p)
        assert same_bits(dvh, r["dense"][p]), (name, p)
        assert same_bits(library.vertical_jvp(*one, units, *c.tail)[1], r["cols"][p]), (name, p)
        if alone_regime[p][0] == c.regime[0]:
            assert same_bits(vjp, r["vjp"][p]), (name, p)
            continue
        live = np.isfinite(vh)
        bound = c.F * 2.0 ** -52 * np.abs(np.where(live[:, None], r["g"][p][:, None] * J, 0.0)).sum(axis=0)
        diff = np.abs(vjp - r["vjp"][p])
        print(f"{name} profile {p}: VJP on {alone_regime[p][0]} waves alone, {c.regime[0]} in the batch: {int((diff > 0).sum())} of "
              f"{c.K[p]} entries differ, largest |difference| / bound {float((diff[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert (diff <= bound).all() and not vjp[c.K[p]:].any(), (name, p)
        reordered += 1
    assert reordered == 1                              # the case is there for it: one profile changes its wave count
    # the same on twelve frequencies that all reflect in the low profile (no truth needed: J's bits are company-free, the
    # VJP is its rows' sum up to the order): J and the JVP keep their bits, the VJP moves, inside the bound
    fo = (orc.plasma_frequency(c.den[0, :c.K[0]]) * 1e-6).max()
    sweep = np.linspace(0.35, 0.95, 12) * fo
    g = np.random.default_rng(7).uniform(-2.0, 2.0, size=(c.P, 12))
    vh_b, J_b, vjp_b, dvh_b = _three((sweep, c.den, c.bmag, c.bpsi, c.alt), g, t, *c.tail)
    vh_a, J_a, vjp_a, dvh_a = _three((sweep, c.den[0], c.bmag[0], c.bpsi[0], c.alt[0]), g[0], t[0], *c.tail)
    assert np.isfinite(vh_b).all() and same_bits(vh_a, vh_b[0]) and same_bits(J_a, J_b[0]) and same_bits(dvh_a, dvh_b[0]), name
    bound = 12 * 2.0 ** -52 * np.abs(g[0][:, None] * J_a).sum(axis=0)
    for got in (vjp_a, vjp_b[0]):                      # each against its rows' sum, then against each other
        want = (g[0].astype(np.longdouble)[:, None] * J_a.astype(np.longdouble)).sum(axis=0)
        assert (np.abs(got.astype(np.longdouble) - want).astype(np.float64) <= bound).all(), name
    diff = np.abs(vjp_a - vjp_b[0])
    moved = int((diff > 0).sum())
    print(f"{name} low profile, 12 reflecting frequencies: {moved} of {c.K[0]} VJP entries differ between four waves (alone) and one "
          f"(batch), largest |difference| / bound {float((diff[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert (diff <= bound).all() and moved > 0, (name, moved)


@pytest.mark.parametrize("bad", dr.BAD_COLUMNS)
@pytest.mark.parametrize("mode,n_points", [("O", 64), ("X", 200)])
def test_a_bad_profile_between_two_clean_ones_leaves_their_bits_alone(g28, column, bad, mode, n_points):
    c, _, t1 = column
    other = {k: g28[f"lo2k_{k}"] for k in ("den", "bmag", "bpsi")}
    assert np.array_equal(other["den"], c["den"])
    second = (c["den"] * 1.25, c["bmag"] * 0.9, c["bpsi"] + 3.0)
    b = dr.bad_column(bad, c["den"], c["bmag"], c["bpsi"], c["alt"])
    assert np.array_equal(b[3], c["alt"], equal_nan=True)
    rng = np.random.default_rng(5)
    g = rng.uniform(-2.0, 2.0, size=(3, c["freq"].size))
    t = np.stack([t1, t1[::-1], 0.5 * t1])
    clean = [np.stack([c[k], c[k], second[i]]) for i, k in enumerate(("den", "bmag", "bpsi"))]
    mixed = [np.stack([c[k], b[i], second[i]]) for i, k in enumerate(("den", "bmag", "bpsi"))]
    want = _three((c["freq"], *clean, c["alt"]), g, t, mode, n_points)
    vh_m = library.vertical_forward_operator(c["freq"], *mixed, c["alt"], mode, n_points)
    g_m = g.copy()
    g_m[1][np.isnan(vh_m[1])] = np.nan                 # (not read)
    got = _three((c["freq"], *mixed, c["alt"]), g_m, t, mode, n_points)
    for a, w in zip(got, want):                        # (vh, J, vjp, dvh), a leading profile axis each
        assert same_bits(a[0], w[0]) and same_bits(a[2], w[2]), bad
    assert same_bits(got[0], vh_m)
    for a in got[1:]:
        assert np.isfinite(a).all(), bad


def test_a_jacobian_row_does_not_depend_on_the_number_of_waves(column):
    """One frequency alone (one wave takes frequencies), with one other (two), among 65 (four): a row is formed by one
    wave from the staged arrays, so its bits are the same.  All frequencies stay above the lowest one of the sweep, so
    the call-wide isotropic decision (magnetised) is the same too."""
    c, _, _ = column
    sweep = np.linspace(1.3, 14.0, 65)
    for mode in "OX":
        for n_points in (64, 200):
            vh, J = library.vertical_jacobian(sweep, c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
            assert np.isfinite(vh).sum() >= 20
            for i in (3, 17, 40):
                assert np.isfinite(vh[i]) and J[i].any()
                vh1, J1 = library.vertical_jacobian(sweep[i:i + 1], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
                vh2, J2 = library.vertical_jacobian(sweep[[i, 50]], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
                assert same_bits(J1[0], J[i]) and same_bits(J2[0], J[i]) and same_bits(J2[1], J[50]), (mode, n_points, i)
                assert same_bits(vh1[0], vh[i]) and same_bits(vh2[0], vh[i])


# ---- f. refusals ---------------------------------------------------------------------------------------------------------
def test_one_level_past_each_limit_is_refused(g28):
    vjp_max, jac_max, jvp_max = (int(x) for x in g28["limits"])

    def column_with_peak_at(level):
        n = level + 3
        alt = 80.0 + 0.2 * np.arange(n)
        den = 1e11 * (1.0 + np.arange(n) / 100.0)
        den[level + 1:] = den[level] * 0.5
        return np.array([4.0, 6.0]), den, np.full(n, 4e-5), np.full(n, 50.0), alt
    args = column_with_peak_at(vjp_max)                # stages vjp_max + 1 levels
    with pytest.raises(ValueError, match=f"the VJP stages at most {vjp_max} levels up to the density peak in LDS; this launch needs {vjp_max + 1} "):
        library.vertical_vjp(*args, np.ones(2), "O", 64)
    args = column_with_peak_at(jac_max)
    with pytest.raises(ValueError, match=f"the Jacobian stages at most {jac_max} levels .* needs {jac_max + 1} "):
        library.vertical_jacobian(*args, "X", 64)
    args = column_with_peak_at(jvp_max)
    with pytest.raises(ValueError, match=f"the JVP stages at most {jvp_max} levels .* needs {jvp_max + 1} "):
        library.vertical_jvp(*args, args[1], "O", 64)
    # ... and the limit itself is taken
    args = column_with_peak_at(vjp_max - 1)
    out = library.vertical_vjp(*args, np.ones(2), "O", 64)
    assert np.isfinite(out).all() and out[:vjp_max - 1].any() and not out[vjp_max - 1:].any()
    args = column_with_peak_at(jac_max - 1)
    vh, J = library.vertical_jacobian(*args, "X", 64)
    vh2, dvh = library.vertical_jvp(*args, args[1], "X", 64)
    assert np.isfinite(vh).all() and same_bits(vh, vh2) and np.isfinite(J).all() and J.any(axis=1).all() and not J[:, jac_max - 1:].any()
    want = (J.astype(np.longdouble) @ args[1].astype(np.longdouble)).astype(np.float64)
    assert (np.abs(dvh - want) <= 1e-9 * (np.abs(J) @ np.abs(args[1]))).all()      # (two kernels, one algorithm: far inside)
