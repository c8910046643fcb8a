"""fitting.trace_sensitivity: S = J D - the operator's analytic Jacobian times central differences of the
smooth profile builder, through one JVP launch - against the float64 restatement tests/vfo_jacobian_numpy.py times the
same D: within 4e-10 max_k |J[f, :]| ||D_i||_1 per entry (the edge-column figure of tests/test_gpu_jacobian.py times
||D_i||_1, over the levels below the peak).  Not compared with finite differences of the operator over the parameters:
on this very column they disagree with J D by 1e-3 ... 3e-2 of the column scale at every step length (the moving grid
crosses a level at almost every step)."""

import copy

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu


def _chapman_builder(F2, F1, E, alt, bottom_type):
    """alpha-Chapman F2 + E layers from the layer dictionaries (the shape of tests/test_gpu_fitting.py's stand-in for the
    reference's PyIRI builders)."""
    thick = F2['B_bot'] if bottom_type == 'B_bot' else F2['B0']
    z = (alt - F2['hm'].ravel()[0]) / thick.ravel()[0]
    ze = (alt - E['hm'].ravel()[0]) / E['B_bot'].ravel()[0]
    return (F2['Nm'].ravel()[0] * np.exp(0.5 * (1.0 - z - np.exp(-z)))
            + E['Nm'].ravel()[0] * np.exp(0.5 * (1.0 - ze - np.exp(-ze))))


def _layer_dicts(nm, hm, bb):
    one = lambda v: np.array([[[v]]])                                           # noqa: E731
    return ({"Nm": one(nm), "hm": one(hm), "B_bot": one(bb)}, {"Nm": one(0.0), "hm": one(200.0), "B_bot": one(30.0)},
            {"Nm": one(3e10), "hm": one(110.0), "B_bot": one(8.0)})


@pytest.mark.parametrize("mode,n_points", [("X", 64), ("O", 200)])
def test_sensitivity_is_the_jacobian_times_the_builders_differences(mode, n_points):
    import vfo_jacobian_numpy as vj
    from oracle import vfo_numpy as orc
    from pyrayhf_amd import fitting, library
    alt = np.arange(80.0, 500.0, 4.0)
    b_mag = 4.6e-5 * ((6371.0 + 80.0) / (6371.0 + alt)) ** 3
    b_psi = 35.0 + 0.002 * (alt - alt[0])
    freq = np.array([1.7, 3.0, 4.5, 6.0, 7.5, 8.6, 12.0])
    values = {"NmF2": 1e12, "hmF2": 301.3, "B_bot": 46.0}
    F2, F1, E = _layer_dicts(values["NmF2"], values["hmF2"], values["B_bot"])
    before = copy.deepcopy((F2, F1, E))
    names = ("NmF2", "hmF2", "B_bot")
    calls = []
    real = library.vertical_jvp

    def counting(*a, **k):
        calls.append(np.asarray(a[5]).shape)
        return real(*a, **k)
    library.vertical_jvp = counting
    try:
        vh, S, edp = fitting.trace_sensitivity(F2, F1, E, freq, alt, b_mag, b_psi, names, mode, n_points, 'B_bot',
                                               edp_builder=_chapman_builder)
    finally:
        library.vertical_jvp = real
    assert calls == [(3, alt.size)]                                             # one launch for all three parameters
    for got, want in zip((F2, F1, E), before):                                  # the inputs are not mutated
        assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) for k in got)
    want_vh, want_edp = fitting.model_VH(F2, F1, E, freq, alt, b_mag, b_psi, mode, n_points, 'B_bot', edp_builder=_chapman_builder)
    assert same_bits(vh, want_vh) and np.array_equal(edp, want_edp)
    assert S.shape == (freq.size, 3) and np.isnan(vh[-1]) and np.isfinite(vh[:-1]).all()

    # the same central differences of the builder, recomputed here
    key = {"NmF2": "Nm", "hmF2": "hm", "B_bot": "B_bot"}
    D = np.empty((3, alt.size))
    for i, name in enumerate(names):
        hi, lo = values[name] * (1.0 + 1e-6), values[name] * (1.0 - 1e-6)
        ends = []
        for v in (hi, lo):
            f2 = copy.deepcopy(F2)
            f2[key[name]] = np.full_like(F2["Nm"], v)
            ends.append(_chapman_builder(f2, F1, E, alt, 'B_bot'))
        D[i] = (ends[0] - ends[1]) / (hi - lo)
    J = vj.jacobian(freq, edp, b_mag, b_psi, alt, mode, orc.stretch_multiplier(n_points))[1]
    K = int(np.argmax(edp))
    want = (J.astype(np.longdouble) @ D.T.astype(np.longdouble)).astype(np.float64)
    bound = 4e-10 * np.abs(J).max(axis=1)[:, None] * np.abs(D[:, :K]).sum(axis=1)[None, :]
    assert not S[-1].any() and not J[-1].any()                                  # the escaping row
    assert (bound[:-1] > 0).all() and S[:-1, 1:].all()          # (NmF2 does not move the E-layer echo at 1.7 MHz)
    ratio = np.abs(S[:-1] - want[:-1]) / bound[:-1]
    print(f"trace_sensitivity {mode} n={n_points}: largest |S - J D| / bound {ratio.max():.3e}; S[2] = {S[2]}")
    assert (ratio <= 1.0).all(), ratio.max()
