"""Host-side checks of fixture g28 (tools/gen_g28_derivative_regimes.py), no GPU: on bad data the float64 restatement
tests/vfo_jacobian_numpy.py has the oracle's NaN mask and values (1e-12 X, 1e-6 O: the tolerances that pin the 50-digit
restatement to the oracle) and the row errors the fixture records; a NaN altitude gives zero, finite rows; the 50-digit
restatement skips NaN terms as the reference's nansum does; and every tall shape lands in the launch regime it is there
for - read from the planning tools (tests/devtools/vjp_plan_host.cpp, jvp_plan_host.cpp), not computed here."""

import shutil

import numpy as np
import pytest

import derivative_regimes as dr
import mp_vfo
import vfo_jacobian_numpy as vj
from conftest import load_golden
from oracle import vfo_numpy as orc

needs_mp = pytest.mark.skipif(not mp_vfo.available(), reason="mpmath is not installed: the 50-digit restatement cannot run")


@pytest.fixture(scope="module")
def g28():
    return load_golden("g28_derivative_regimes.npz")


@pytest.fixture(scope="module")
def e26():
    g = load_golden("g26_jacobian.npz")
    return {"O": float(g["e_ref_O"]), "X": float(g["e_ref_X"])}


def cases(g, kind=None):
    for name in g["cases"]:
        name = str(name)
        if kind is None or dr.kind_of(g, name) == kind:
            yield name, {k: g[f"{name}_{k}"] for k in dr.KEYS}, str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])


def profiles(c):
    """(p, den, bmag, bpsi, alt, vh_mp, jac_mp) per profile of a case (a batch has a leading axis)."""
    if c["den"].ndim == 1:
        yield 0, c["den"], c["bmag"], c["bpsi"], c["alt"], c["vh_mp"], c["jac_mp"]
    else:
        for p in range(c["den"].shape[0]):
            yield p, c["den"][p], c["bmag"][p], c["bpsi"][p], c["alt"][p], c["vh_mp"][p], c["jac_mp"][p]


def test_fixture_holds_the_cases_of_every_kind(g28):
    names = [str(n) for n in g28["cases"]]
    assert [n for n in names if n.startswith("t")] == ["t1a", "t1b", "t2a", "t2b", "t3a", "t3b", "t4a", "t4b", "t5a", "t5b"]
    assert {n for n in names if n.startswith("l")} == {"lx20k", "lx2k", "lo2k", "lo2k620"}
    assert {n for n in names if dr.kind_of(g28, n) == "bad"} == \
        {f"{col}_{mode}{n}" for col in dr.BAD_COLUMNS for mode in "OX" for n in (64, 200)}
    assert int(g28["lx20k_n_points"]) == 20000 and g28["lx20k_freq"].size == 3 and g28["lo2k620_den"].size == 620
    tall = list(cases(g28, "tall"))
    assert {m for _, _, m, _ in tall} == {"O", "X"} and {n for _, _, _, n in tall} == {64, 65, 200}
    for name, c, mode, n_points in cases(g28):
        assert c["jac_mp"].shape[-1] == dr.highest_peak(c["den"]), name
        if dr.kind_of(g28, name) == "bad":
            assert c["freq"].size == 5 and c["den"].size == 78
        for p, den, bmag, bpsi, alt, vh_mp, jac_mp in profiles(c):
            assert np.isfinite(jac_mp).all() and not jac_mp[np.isnan(vh_mp)].any(), name
            assert not jac_mp[:, int(np.argmax(den)):].any(), name
            assert np.isnan(alt).any() or (np.diff(alt) > 0).all(), name
            if dr.kind_of(g28, name) != "bad":          # every profile, those of a batch too, has pairs with a value and a row
                assert np.isfinite(vh_mp).sum() >= 2 and jac_mp.any(axis=1).sum() >= 2 and np.isnan(vh_mp).any(), (name, p)
    # the bad-data truths the issue names: |B| NaN in X mode is an all-NaN trace, everything else keeps some pairs
    for n in (64, 200):
        assert np.isnan(g28[f"bmid_X{n}_vh_mp"]).all() and np.isfinite(g28[f"bmid_O{n}_vh_mp"]).any()
        for col in ("psimid", "psi0", "denmid", "denext"):
            for mode in "OX":
                assert np.isfinite(g28[f"{col}_{mode}{n}_vh_mp"]).sum() >= 2, (col, mode, n)
    assert int(np.argmax(g28["denmid_O64_den"])) == 18 and int(np.argmax(g28["denext_O64_den"])) == 40     # K/2 and K + 3


def test_restatement_matches_the_oracle_on_bad_data_and_reproduces_the_recorded_errors(g28, e26):
    worst28 = {"O": 0.0, "X": 0.0}
    own = {str(n) for n in g28["own_e_ref"]}
    for name, c, mode, n_points in cases(g28):
        kind = dr.kind_of(g28, name)
        if n_points > 2000:
            continue                                   # (the 20 000-point restatement builds a dense (n, K) array: the generator's job)
        worst = 0.0
        for p, den, bmag, bpsi, alt, vh_mp, jac_mp in profiles(c):
            with np.errstate(all="ignore"), np.testing.suppress_warnings() as sup:
                sup.filter(RuntimeWarning)
                want = orc.virtual_heights(c["freq"], den, bmag, bpsi, alt, mode, n_points)
                vh, J = vj.jacobian(c["freq"], den, bmag, bpsi, alt, mode, orc.stretch_multiplier(n_points))
            assert np.array_equal(np.isnan(vh), np.isnan(want)) and np.array_equal(np.isnan(vh_mp), np.isnan(want)), name
            ok = np.isfinite(want)
            tol = 1e-12 if mode == "X" else 1e-6
            if ok.any():
                if kind == "bad":                      # (elsewhere the float64 restatement's value is not what is pinned)
                    assert (np.abs(vh[ok] - want[ok]) <= tol * np.abs(want[ok])).all(), (name, vh, want)
                assert (np.abs(vh_mp[ok] - want[ok]) <= tol * np.abs(want[ok])).all(), (name, vh_mp, want)
            assert np.isfinite(J).all() and not J[~ok].any(), name
            K = jac_mp.shape[-1]
            assert not J[:, K:].any(), name
            for i in range(c["freq"].size):
                scale = np.abs(jac_mp[i]).max()
                if scale:
                    worst = max(worst, float(np.abs(J[i, :K] - jac_mp[i]).max() / scale))
        if kind == "bad":
            worst28[mode] = max(worst28[mode], worst)
        if name in own:
            assert e26[mode] < worst <= float(g28[f"{name}_e_ref"]) * (1 + 1e-12), (name, worst)
        else:
            assert worst <= e26[mode], (name, worst)
    for mode in "OX":
        assert worst28[mode] <= float(g28[f"e_ref28_{mode}"]) * (1 + 1e-12) and float(g28[f"e_ref28_{mode}"]) <= e26[mode]


def test_isotropic_decision_ignores_a_nan_field(g28):
    """|B| 1e-12 of its size with one NaN: np.nanmax|Y| < 1e-12 - O mode takes the isotropic branch (with np.max it
    would not), and the restatements agree with the oracle there (above)."""
    c = {k: g28[f"btiny_O64_{k}"] for k in dr.KEYS}
    K = int(np.argmax(c["den"]))
    assert np.isnan(c["bmag"][:K]).sum() == 1
    assert vj.unmagnetised(c["freq"], c["bmag"][:K]) and mp_vfo.unmagnetised(c["freq"], c["den"], c["bmag"])
    assert not vj.unmagnetised(c["freq"], g28["bmid_O64_bmag"][:K])
    assert not vj.unmagnetised(c["freq"], np.full(K, np.nan)) and not mp_vfo.unmagnetised(c["freq"], c["den"], np.full(78, np.nan))


@pytest.mark.parametrize("level", ["below", "above"])
def test_a_nan_altitude_gives_nan_heights_and_zero_finite_rows(g28, level):
    c = {k: g28[f"lx2k_{k}"] for k in dr.KEYS}
    K = int(np.argmax(c["den"]))
    alt = c["alt"].copy()
    alt[K // 2 if level == "below" else K + 3] = np.nan
    for mode in "OX":
        with np.errstate(all="ignore"):
            want = orc.virtual_heights(c["freq"], c["den"], c["bmag"], c["bpsi"], alt, mode, 64)
            vh, J = vj.jacobian(c["freq"], c["den"], c["bmag"], c["bpsi"], alt, mode, orc.stretch_multiplier(64))
        assert np.isnan(want).all() and np.isnan(vh).all() and np.isfinite(J).all() and not J.any()
        if mp_vfo.available():
            v, row = mp_vfo.jacobian_row(c["freq"][1], c["den"], c["bmag"], c["bpsi"], alt, mode, orc.stretch_multiplier(64))
            assert np.isnan(v) and not row.any()


@needs_mp
def test_mp_rows_with_skipped_terms_are_reproduced(g28):
    """One row each of a column whose sum skips NaN terms (psi NaN at K/2), of the nanmax column and of the extended
    bottomside; and the skipped terms are there: the same pair on the clean column has another value."""
    for name, i in (("psimid_X64", 2), ("btiny_O64", 3), ("denext_O64", 1)):
        c = {k: g28[f"{name}_{k}"] for k in dr.KEYS}
        mode = str(g28[f"{name}_mode"])
        mult = orc.stretch_multiplier(64)
        unmag = mp_vfo.unmagnetised(c["freq"], c["den"], c["bmag"])
        vh, row = mp_vfo.jacobian_row(c["freq"][i], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, mult, unmag)
        assert np.isfinite(vh) and vh == c["vh_mp"][i] and np.array_equal(row[:c["jac_mp"].shape[1]], c["jac_mp"][i]), name
    c = {k: g28[f"psimid_X64_{k}"] for k in dr.KEYS}
    clean = mp_vfo.virtual_height(c["freq"][2], c["den"], c["bmag"], g28["lx2k_bpsi"], c["alt"], "X", orc.stretch_multiplier(64))
    assert np.isfinite(clean) and clean > c["vh_mp"][2]


# ---- regimes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return dr.build_tools(tmp_path_factory.mktemp("plan_tools"))


def test_every_case_lands_in_its_recorded_regime(g28, tools):
    for name, c, mode, n_points in cases(g28):
        P = 1 if c["den"].ndim == 1 else c["den"].shape[0]
        peak = dr.highest_peak(c["den"])
        got = dr.regime(tools, P, c["freq"].size, c["den"].shape[-1], peak, dr.n_unit(dr.kind_of(g28, name), peak))
        assert np.array_equal(got, g28[f"{name}_regime"]), (name, got, g28[f"{name}_regime"])
        if P > 1:
            alone = np.stack([dr.regime(tools, 1, c["freq"].size, c["den"].shape[-1], int(np.argmax(d))) for d in c["den"]])
            assert np.array_equal(alone, g28[f"{name}_regime_alone"]), name


def test_tall_cases_hit_the_regimes_they_are_meant_to(g28, tools):
    """[VJP waves, VJP levels, Jacobian waves, Jacobian levels, JVP chunk (24 tangents), JVP levels, JVP chunk (3 tangents)]"""
    vjp_max, jac_max, jvp_max = dr.limits(tools)
    assert g28["limits"].tolist() == [vjp_max, jac_max, jvp_max]
    reg = {n: g28[f"{n}_regime"].tolist() for n in ("t1a", "t1b", "t2a", "t2b", "t3a", "t3b", "t4a", "t4b", "t5a", "t5b")}
    for n in ("t1a", "t1b"):                           # VJP on two waves; JVP chunk 4; the whole column staged
        assert reg[n] == [2, 1000, 4, 1000, 4, 1000, 4], reg[n]
    for n in ("t2a", "t2b"):                           # VJP on one wave; JVP chunk 2
        assert reg[n][0] == 1 and reg[n][4] == 2 == reg[n][6] and reg[n][1:6:2] == [1200, 1200, 1200], reg[n]
    for n in ("t3a", "t3b"):                           # VJP through the pre-pass to L = 1241; Jacobian and JVP stage all 1300
        assert reg[n] == [1, 1241, 1, 1300, 1, 1300, 1], reg[n]
        assert vjp_max < 1300 <= min(jac_max, jvp_max) and 1241 <= vjp_max
    for n in ("t4a", "t4b"):                           # all three through the pre-pass
        assert reg[n][1:6:2] == [1001, 1001, 1001] and 1400 > max(vjp_max, jac_max, jvp_max) and 0 not in reg[n], reg[n]
    for n in ("t5a", "t5b"):                           # staged for the higher of the two peaks
        assert reg[n][1:6:2] == [1201, 1201, 1201] and 0 not in reg[n], reg[n]
        # alone, the low profile is staged for its own 301 levels on four waves and chunks of eight: the VJP adds its
        # frequencies in another order there than in the batch (one wave); the high profile's launch is the batch's
        assert g28[f"{n}_regime_alone"].tolist() == [[4, 301, 4, 301, 8, 301, 4], reg[n]], n
        assert g28[f"{n}_freq"].size > 4                # (more frequencies than waves: the order does differ)
        assert sorted(int(np.argmax(d)) for d in g28[f"{n}_den"]) == [300, 1200]
    # more levels than the hint table has buckets in every tall case; one level past a limit is refused
    assert all(r[1] > 1024 or n.startswith("t1") or n.startswith("t4") for n, r in reg.items())
    assert dr.regime(tools, 1, 2, vjp_max + 1, vjp_max)[0] == 0 and dr.regime(tools, 1, 2, vjp_max, vjp_max - 1)[0] == 1
    assert dr.regime(tools, 1, 2, jac_max + 1, jac_max)[2] == 0 and dr.regime(tools, 1, 2, jvp_max + 1, jvp_max)[4] == 0
    assert (vjp_max, jac_max, jvp_max) == (1249, 1332, 1332)           # the documented figures (include/prhf.h)
