"""The JVP kernel (prhf_vfo_jvp_f64) against the 50-digit Jacobians of fixture g26.

The Jacobian kernels are held to 4 e_ref[mode] max_k |J_mp[f, :]| per entry (tests/test_gpu_jacobian.py; e_ref: the
float64 restatement's distance from the truth, pinned in the fixture).  A dot product of such a row with a tangent t
inherits at worst 4 e_ref max_k |J_mp[f, :]| ||t||_1 - the bound used here, with ||t||_1 over the levels below the
density peak (the only ones J is non-zero at); the restatement's own J @ t stays inside it by the definition of e_ref.
Nothing is compared with finite differences of the operator (they do not converge).  The measured ratios
are appended to profiles/jacobian_parity.md."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity_report import put_section
from pyrayhf_amd import library, synth

pytestmark = pytest.mark.gpu

HEADING = "# JVP kernel against the 50-digit truth (fixture g26)"


def cases(g):
    for name in g["cases"]:
        name = str(name)
        yield name, {k: g[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt", "vh_mp", "jac_mp")}, \
            str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])


@pytest.fixture(scope="module")
def g26():
    return load_golden("g26_jacobian.npz")


def dense_tangents(c, seed=26):
    """T = 3 directions den * u, u uniform in (-1, 1)."""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(3, c["den"].size))
    return c["den"][None, :] * u


@pytest.fixture(scope="module")
def computed(g26):
    """name -> (vh, dvh along every unit vector below the peak, dvh along the three dense directions)."""
    out = {}
    for name, c, mode, n_points in cases(g26):
        K = int(np.argmax(c["den"]))
        units = np.eye(c["den"].size)[:K]
        vh, cols = library.vertical_jvp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], units, mode, n_points)
        vh2, dense = library.vertical_jvp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], dense_tangents(c), mode, n_points)
        assert same_bits(vh, vh2)
        out[name] = (vh, cols, dense)
    return out


def _append_table(lines):
    """Put the section under HEADING into profiles/jacobian_parity.md; the other sections stay (an earlier copy of this
    one is replaced)."""
    put_section(lines)


def test_every_jacobian_column_within_the_jacobian_kernels_bound(g26, computed):
    e_ref = {"O": float(g26["e_ref_O"]), "X": float(g26["e_ref_X"])}
    lines = [HEADING, "",
             "Tangents: the K = argmax den unit vectors (19 ... 195 per case: chunks of 8 and a remainder).  err = "
             "max_k |dvh[f, k] - J_mp[f, k]| / max_k |J_mp[f, :]| per row; bound 4 x e_ref[mode].  Written by tests/test_gpu_jvp.py.",
             "", "| case | mode | n_points | levels | T | worst row err | err / e_ref |", "|---|---|---|---|---|---|---|"]
    worst = {"O": 0.0, "X": 0.0}
    failures = []
    for name, c, mode, n_points in cases(g26):
        vh, cols, _ = computed[name]
        K = int(np.argmax(c["den"]))
        assert K > 8, (name, K)
        assert cols.shape == (c["freq"].size, K) and np.isfinite(cols).all(), name
        assert np.array_equal(np.isnan(vh), np.isnan(c["vh_mp"])), name
        case_worst = 0.0
        for i, f in enumerate(c["freq"]):
            scale = np.abs(c["jac_mp"][i]).max()
            if scale == 0.0:
                continue
            err = float(np.abs(cols[i] - c["jac_mp"][i, :K]).max() / scale)
            case_worst = max(case_worst, err)
            if not err <= 4.0 * e_ref[mode]:
                failures.append((name, i, err))
        worst[mode] = max(worst[mode], case_worst)
        lines.append(f"| {name} | {mode} | {n_points} | {c['den'].size} | {K} | {case_worst:.3e} | {case_worst / e_ref[mode]:.2f} |")
        print(f"jvp columns {name} {mode} n={n_points} T={K}: err {case_worst:.3e} ({case_worst / e_ref[mode]:.2f} x e_ref)")
    lines += ["", f"Worst: O {worst['O']:.3e} ({worst['O'] / e_ref['O']:.2f} x e_ref), "
              f"X {worst['X']:.3e} ({worst['X'] / e_ref['X']:.2f} x e_ref)."]
    print(lines[-1])
    _append_table(lines)
    assert not failures, failures


def test_dense_directions_within_the_bound_of_a_dot_product(g26, computed):
    e_ref = {"O": float(g26["e_ref_O"]), "X": float(g26["e_ref_X"])}
    worst = {"O": 0.0, "X": 0.0}
    for name, c, mode, n_points in cases(g26):
        _, _, dense = computed[name]
        K = int(np.argmax(c["den"]))
        t = dense_tangents(c)
        want = c["jac_mp"].astype(np.longdouble) @ t.astype(np.longdouble).T                 # (F, 3)
        norm1 = np.abs(t[:, :K]).sum(axis=1)                                                 # (3,)
        bound = 4.0 * e_ref[mode] * np.abs(c["jac_mp"]).max(axis=1)[:, None] * norm1[None, :]
        assert dense.shape == want.shape == (c["freq"].size, 3) and np.isfinite(dense).all(), name
        diff = np.abs(dense.astype(np.longdouble) - want).astype(np.float64)
        live = bound > 0
        assert live.any() and not dense[~live].any(), name
        worst[mode] = max(worst[mode], float((diff[live] / bound[live]).max()))
        assert (diff <= bound).all(), (name, float((diff[live] / bound[live]).max()))
    print(f"jvp dense directions: largest |dvh - J_mp t| / bound  O {worst['O']:.3f}  X {worst['X']:.3f}")


def test_adjoint_identity_with_the_vjp(g26, computed):
    e_ref = {"O": float(g26["e_ref_O"]), "X": float(g26["e_ref_X"])}
    worst = 0.0
    for n, (name, c, mode, n_points) in enumerate(cases(g26)):
        vh, _, dense = computed[name]
        K = int(np.argmax(c["den"]))
        t = dense_tangents(c)
        g = np.random.default_rng(100 + n).uniform(-2.0, 2.0, size=c["freq"].size)
        g[~np.isfinite(vh)] = 0.0
        back = library.vertical_vjp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], g, mode, n_points)
        lhs = (g.astype(np.longdouble)[:, None] * dense.astype(np.longdouble)).sum(axis=0)       # (3,)
        rhs = t.astype(np.longdouble) @ back.astype(np.longdouble)
        bound = 8.0 * e_ref[mode] * float((np.abs(g) * np.abs(c["jac_mp"]).max(axis=1)).sum()) * np.abs(t[:, :K]).sum(axis=1)
        ratio = float((np.abs(lhs - rhs).astype(np.float64) / bound).max())
        print(f"adjoint identity {name} {mode} n={n_points}: |<g, J t> - <J^T g, t>| / bound {ratio:.3e}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    print(f"adjoint identity: worst ratio {worst:.3e}")


def test_conventions(g26, computed):
    escaping = 0
    for name, c, mode, n_points in cases(g26):
        vh, cols, dense = computed[name]
        esc = np.isnan(vh)
        escaping += int(esc.sum())
        assert not cols[esc].any() and not dense[esc].any(), name                    # exact zeros
        assert cols[~esc].any(axis=1).all(), name
        want = library.vertical_forward_operator(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
        assert same_bits(vh, want), name
        K = int(np.argmax(c["den"]))
        dirty = dense_tangents(c)
        dirty[:, K:] = np.nan
        vh2, got = library.vertical_jvp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], dirty, mode, n_points)
        assert same_bits(got, dense) and np.isfinite(got).all() and same_bits(vh2, vh), name
    assert escaping >= 10


# ---- bits do not depend on company ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    alt, den, bmag, bpsi = synth.chapman_profiles(24, 41)
    rows = [3, 11, 17]
    alt, den, bmag, bpsi = alt[::8].copy(), den[rows, ::8].copy(), bmag[rows, ::8].copy(), bpsi[rows, ::8].copy()
    tangents = den[:, None, :] * np.random.default_rng(9).uniform(-1.0, 1.0, size=(3, 9, alt.size))
    return alt, den, bmag, bpsi, tangents


def sweep(n_freq):
    return np.array([4.1]) if n_freq == 1 else np.linspace(1.3, 14.0, n_freq)


@pytest.mark.parametrize("mode,n_points", [("O", 63), ("X", 64), ("O", 200)])
@pytest.mark.parametrize("n_freq", [1, 4, 5, 9])        # fewer than the waves, one each, eight waves, a second round
def test_a_column_does_not_depend_on_the_other_tangents(batch, mode, n_points, n_freq):
    alt, den, bmag, bpsi, tangents = batch
    freq = sweep(n_freq)
    vh, all9 = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents, mode, n_points)
    assert all9.shape == (3, n_freq, 9) and np.isfinite(all9).all() and all9[np.isfinite(vh)].any(axis=1).all()
    for t in range(9):
        vh1, alone = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[:, t], mode, n_points)
        assert alone.shape == vh.shape and same_bits(alone, all9[:, :, t]) and same_bits(vh1, vh), (t, mode)
    pick = [5, 2, 8]
    three = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[:, pick], mode, n_points)[1]
    assert three.shape == (3, n_freq, 3) and same_bits(three, all9[:, :, pick])
    eight = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[:, 1:], mode, n_points)[1]
    assert same_bits(eight, all9[:, :, 1:])
    again = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents, mode, n_points)[1]
    assert same_bits(again, all9)
    for p in range(3):
        vh_p, alone = library.vertical_jvp(freq, den[p], bmag[p], bpsi[p], alt, tangents[p], mode, n_points)
        assert alone.shape == (n_freq, 9) and same_bits(alone, all9[p]) and same_bits(vh_p, vh[p]), (p, mode)


def test_numpy_and_torch_resident_inputs_give_equal_bits(batch):
    import torch
    alt, den, bmag, bpsi, tangents = batch
    freq = sweep(5)
    t = lambda x: torch.as_tensor(x, device="cuda")     # noqa: E731
    for mode in "OX":
        vh_h, host = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents, mode, 65)
        vh_d, dev = library.vertical_jvp(t(freq), t(den), t(bmag), t(bpsi), t(alt), t(tangents), mode, 65)
        assert torch.is_tensor(dev) and dev.is_cuda and same_bits(dev.cpu().numpy(), host)
        assert same_bits(vh_d.cpu().numpy(), vh_h)
        one = library.vertical_jvp(t(freq), t(den[1]), t(bmag[1]), t(bpsi[1]), t(alt), t(tangents[1, 4]), mode, 65)[1]
        assert tuple(one.shape) == (5,) and same_bits(one.cpu().numpy(), host[1, :, 4])


def test_shared_tangents_and_shared_fields(batch):
    alt, den, bmag, bpsi, tangents = batch
    freq = sweep(5)
    for mode in "OX":
        shared = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[0], mode, 64, shared=True)[1]
        tiled = library.vertical_jvp(freq, den, bmag, bpsi, alt, np.tile(tangents[0], (3, 1, 1)), mode, 64)[1]
        assert shared.shape == (3, 5, 9) and same_bits(shared, tiled) and shared.any()
        one = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[0, 3], mode, 64, shared=True)[1]
        assert one.shape == (3, 5) and same_bits(one, shared[:, :, 3])
        field = library.vertical_jvp(freq, den, bmag[0], bpsi[0], alt, tangents, mode, 64)[1]
        tiled = library.vertical_jvp(freq, den, np.tile(bmag[0], (3, 1)), np.tile(bpsi[0], (3, 1)), alt, tangents, mode, 64)[1]
        assert same_bits(field, tiled) and field.any()


# ---- edge columns --------------------------------------------------------------------------------------------------------
def test_edge_columns_agree_with_the_float64_restatement():
    """The six columns of tests/test_gpu_jacobian.py's edge test - a grid that collapses onto level 0, a one-level
    bottomside, a one-point grid, each in both modes - with two dense tangents against tests/vfo_jacobian_numpy.py's
    J @ t: within 4e-10 max_k |J[f, :]| ||t||_1 (that test's figure times ||t||_1); zero rows give exact zeros."""
    import vfo_jacobian_numpy as vj
    from oracle import vfo_numpy as orc
    alt, den, bmag, bpsi = synth.chapman_profiles(8, 77)
    alt, den, bmag, bpsi = alt[::8].copy(), den[2, ::8].copy(), bmag[2, ::8].copy(), bpsi[2, ::8].copy()
    K = int(np.argmax(den))
    fn0 = 8.97866275e-6 * np.sqrt(den[0])
    fo = 8.97866275e-6 * np.sqrt(den[:K].max())
    one_level = den.copy()
    one_level[1] = 2.0 * den.max()                      # the peak at level 1: K = 1
    columns = [("collapsed O", den, "O", 64, np.array([0.5 * fn0, 0.6 * fo, 2.0 * fo])),
               ("collapsed X", den, "X", 64, np.array([0.3, 0.9, 0.6 * fo, 2.0 * fo])),
               ("one level O", one_level, "O", 63, np.array([0.5 * fn0, 2.0 * fn0, 5.0])),
               ("one level X", one_level, "X", 65, np.array([0.5, 3.0])),
               ("one point", den, "O", 1, np.array([0.5 * fo, 0.9 * fo, 2.0 * fo])),
               ("one point X", den, "X", 1, np.array([0.5 * fo, 0.9 * fo]))]
    checked = zero_rows = 0
    for name, d, mode, n_points, freq in columns:
        Kd = int(np.argmax(d))
        t = d[None, :] * np.random.default_rng(5).uniform(-1.0, 1.0, size=(2, d.size))
        vh, dvh = library.vertical_jvp(freq, d, bmag, bpsi, alt, t, mode, n_points)
        _, J = vj.jacobian(freq, d, bmag, bpsi, alt, mode, orc.stretch_multiplier(n_points))
        want = J.astype(np.longdouble) @ t.astype(np.longdouble).T
        assert dvh.shape == (freq.size, 2) and np.isfinite(dvh).all(), name
        for i in range(freq.size):
            scale = np.abs(J[i]).max()
            if scale == 0.0:
                assert not dvh[i].any(), (name, i)
                zero_rows += 1
                continue
            assert np.isfinite(vh[i]), (name, i)
            bound = 4e-10 * scale * np.abs(t[:, :Kd]).sum(axis=1)
            err = np.abs(dvh[i].astype(np.longdouble) - want[i]).astype(np.float64)
            print(f"edge column {name} f={freq[i]:.4f}: |dvh - J t| / bound {float((err / bound).max()):.3e}")
            assert (err <= bound).all(), (name, i, err, bound)
            checked += 1
    assert checked >= 6 and zero_rows >= 4


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_call(batch):
    n = 3000
    alt = 80.0 + 0.2 * np.arange(n)
    den = 1e11 * (1.0 + np.arange(n) / 100.0)
    den[2600:] = den[2599] * 0.5                       # the peak at level 2599: 2600 levels to stage
    bmag, bpsi = np.full(n, 4e-5), np.full(n, 50.0)
    freq = np.array([3.0, 5.0])
    with pytest.raises(ValueError, match="the JVP stages at most 1332 levels"):
        library.vertical_jvp(freq, den, bmag, bpsi, alt, den, "O", 64)
    # ... while a long column whose bottomside fits is taken (the peak pre-pass): 1000 levels, past eight columns' room
    den2 = den.copy()
    den2[1000:] = den2[999] * 0.5
    t = np.stack([den2 * 0.5, -den2, den2 * np.cos(np.arange(n))])
    vh, dvh = library.vertical_jvp(freq, den2, bmag, bpsi, alt, t, "O", 64)
    assert dvh.shape == (2, 3) and np.isfinite(vh).all() and dvh.all()
    assert same_bits(dvh[:, 1], library.vertical_jvp(freq, den2, bmag, bpsi, alt, t[1], "O", 64)[1])
    import vfo_jacobian_numpy as vj
    from oracle import vfo_numpy as orc
    J = vj.jacobian(freq, den2, bmag, bpsi, alt, "O", orc.stretch_multiplier(64))[1]
    bound = 4e-10 * np.abs(J).max(axis=1)[:, None] * np.abs(t[:, :999]).sum(axis=1)[None, :]     # (the edge columns' figure)
    assert (np.abs(dvh - (J.astype(np.longdouble) @ t.T.astype(np.longdouble)).astype(np.float64)) <= bound).all()

    alt, den, bmag, bpsi, tangents = batch
    freq = sweep(4)
    for bad in (tangents[:2], tangents[:, :, :-1], tangents[0, 0, :-1], tangents[None]):
        with pytest.raises(ValueError, match="tangents"):
            library.vertical_jvp(freq, den, bmag, bpsi, alt, bad, "X", 64)
    with pytest.raises(ValueError, match="shared tangents"):
        library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents, "X", 64, shared=True)
    vh, empty = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangents[:, :0], "X", 64)
    assert empty.shape == (3, 4, 0) and same_bits(vh, library.vertical_forward_operator(freq, den, bmag, bpsi, alt, "X", 64))
    vh, empty = library.vertical_jvp(freq, den[0], bmag[0], bpsi[0], alt, tangents[0, :0], "O", 64)
    assert empty.shape == (4, 0) and vh.shape == (4,)
