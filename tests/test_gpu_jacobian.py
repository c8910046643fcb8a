"""The Jacobian kernels (prhf_vfo_jacobian_f64) against the 50-digit truth of fixture g26
(tools/gen_g26_jacobian.py): per row err = max_k |J - J_mp| / max_k |J_mp| <= 4 x e_ref[mode], where e_ref is the largest
such error of the float64 NumPy restatement (tests/vfo_jacobian_numpy.py) - the factor 4 covers another math library's
last bits, not another algorithm.  Every row of the fixture is checked.  The measured errors go to
profiles/jacobian_parity.md."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity_report import put_section
from pyrayhf_amd import library

pytestmark = pytest.mark.gpu


def cases(g):
    for name in g["cases"]:
        name = str(name)
        yield name, {k: g[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt", "vh_mp", "jac_mp")}, \
            str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])


@pytest.fixture(scope="module")
def g26():
    return load_golden("g26_jacobian.npz")


@pytest.fixture(scope="module")
def computed(g26):
    """name -> (vh, J) of one vertical_jacobian call per fixture case."""
    return {name: library.vertical_jacobian(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
            for name, c, mode, n_points in cases(g26)}


def test_every_row_within_four_times_the_float64_restatement(g26, computed):
    e_ref = {"O": float(g26["e_ref_O"]), "X": float(g26["e_ref_X"])}
    lines = ["# Jacobian kernels against the 50-digit truth (fixture g26)", "",
             "err = max_k |J - J_mp| / max_k |J_mp| per row; bound 4 x e_ref[mode], e_ref = the float64 NumPy restatement's "
             f"largest err: O {e_ref['O']:.3e}, X {e_ref['X']:.3e}.  Written by tests/test_gpu_jacobian.py.", "",
             "| case | mode | n_points | levels | f [MHz] | err | err / e_ref |", "|---|---|---|---|---|---|---|"]
    worst = {"O": 0.0, "X": 0.0}
    failures = []
    for name, c, mode, n_points in cases(g26):
        vh, J = computed[name]
        assert J.shape == c["jac_mp"].shape and np.array_equal(np.isnan(vh), np.isnan(c["vh_mp"])), name
        for i, f in enumerate(c["freq"]):
            scale = np.abs(c["jac_mp"][i]).max()
            if scale == 0.0:
                continue
            err = float(np.abs(J[i] - c["jac_mp"][i]).max() / scale)
            worst[mode] = max(worst[mode], err)
            lines.append(f"| {name} | {mode} | {n_points} | {c['den'].size} | {f:.4f} | {err:.3e} | {err / e_ref[mode]:.2f} |")
            print(f"jacobian parity {name} {mode} n={n_points} f={f:.4f}: err {err:.3e} ({err / e_ref[mode]:.2f} x e_ref)")
            if not err <= 4.0 * e_ref[mode]:
                failures.append((name, i, err))
    lines += ["", f"Worst: O {worst['O']:.3e} ({worst['O'] / e_ref['O']:.2f} x e_ref), "
              f"X {worst['X']:.3e} ({worst['X'] / e_ref['X']:.2f} x e_ref)."]
    put_section(lines, first=True)                     # (the other files' sections of the report stay)
    assert not failures, failures


def test_rows_of_pairs_without_a_value_and_levels_above_the_peak_are_zero(g26, computed):
    escaping = 0
    for name, c, mode, n_points in cases(g26):
        vh, J = computed[name]
        K = int(np.argmax(c["den"]))
        assert not J[:, K:].any(), name
        assert not J[np.isnan(vh)].any(), name
        assert np.isfinite(J).all(), name
        escaping += int(np.isnan(vh).sum())
        assert J[np.isfinite(vh)].any(axis=1).all(), name
    assert escaping >= 10


def test_vh_equals_the_operator_bit_for_bit(g26, computed):
    for name, c, mode, n_points in cases(g26):
        want = library.vertical_forward_operator(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
        assert same_bits(computed[name][0], want), name


def test_nan_upstream_gradient_at_an_escaping_pair_changes_nothing(g26):
    for name in ("g", "h"):
        c = {k: g26[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt", "vh_mp")}
        mode, n_points = str(g26[f"{name}_mode"]), int(g26[f"{name}_n_points"])
        esc = np.isnan(c["vh_mp"])
        assert esc.any() and not esc.all()
        g = np.linspace(-1.0, 2.0, c["freq"].size)
        g[esc] = 0.0
        clean = library.vertical_vjp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], g, mode, n_points)
        g[esc] = np.nan
        dirty = library.vertical_vjp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], g, mode, n_points)
        assert np.isfinite(dirty).all() and dirty.any() and np.array_equal(clean, dirty), name


def test_edge_columns_agree_with_the_float64_restatement():
    """Columns off the fixture's beaten track - a one-level bottomside, a grid that collapses onto level 0 (c_0 > 1: the
    frequency below the bottom level's plasma frequency in O mode, below its gyrofrequency in X mode), a one-point grid, a
    plateau in the running maximum's argmax excluded - against tests/vfo_jacobian_numpy.py, the same algorithm in
    float64: within 4e-10 of the row scale (4 x the restatement's own distance from the truth on the fixture, 8.9e-11),
    equal zero rows, and the operator's NaN mask wherever a row is non-zero."""
    import vfo_jacobian_numpy as vj
    from oracle import vfo_numpy as orc
    from pyrayhf_amd import synth
    alt, den, bmag, bpsi = synth.chapman_profiles(8, 77)
    alt, den, bmag, bpsi = alt[::8].copy(), den[2, ::8].copy(), bmag[2, ::8].copy(), bpsi[2, ::8].copy()
    K = int(np.argmax(den))
    fn0 = 8.97866275e-6 * np.sqrt(den[0])
    fo = 8.97866275e-6 * np.sqrt(den[:K].max())
    one_level = den.copy()
    one_level[1] = 2.0 * den.max()                      # the peak at level 1: K = 1
    columns = [("collapsed O", den, "O", 64, np.array([0.5 * fn0, 0.6 * fo, 2.0 * fo])),
               ("collapsed X", den, "X", 64, np.array([0.3, 0.9, 0.6 * fo, 2.0 * fo])),     # f_H ~ 1 MHz: X + Y > 1 at level 0
               ("one level O", one_level, "O", 63, np.array([0.5 * fn0, 2.0 * fn0, 5.0])),
               ("one level X", one_level, "X", 65, np.array([0.5, 3.0])),
               ("one point", den, "O", 1, np.array([0.5 * fo, 0.9 * fo, 2.0 * fo])),
               ("one point X", den, "X", 1, np.array([0.5 * fo, 0.9 * fo]))]
    checked = 0
    for name, d, mode, n_points, freq in columns:
        vh, J = library.vertical_jacobian(freq, d, bmag, bpsi, alt, mode, n_points)
        want_vh, want = vj.jacobian(freq, d, bmag, bpsi, alt, mode, orc.stretch_multiplier(n_points))
        assert np.isfinite(J).all() and J.shape == want.shape, name
        for i in range(freq.size):
            scale = np.abs(want[i]).max()
            if scale == 0.0:
                assert not J[i].any(), (name, i)
                continue
            assert np.isfinite(vh[i]), (name, i)
            err = np.abs(J[i] - want[i]).max() / scale
            print(f"edge column {name} f={freq[i]:.4f}: err {err:.3e}")
            assert err <= 4e-10, (name, i, err)
            checked += 1
    assert checked >= 6
