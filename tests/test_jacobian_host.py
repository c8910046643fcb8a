"""Host-side checks of the operator's derivative, no GPU: the 50-digit restatement tests/mp_vfo.py is
pinned to the oracle's values and to finite differences of the reference's own operator (recorded in fixture g26 by
tools/gen_g26_jacobian.py); the float64 restatement tests/vfo_jacobian_numpy.py reproduces the recorded ``e_ref``; the two
new C symbols are declared, bound and exported; the launch planning of the new kernels (plan_vjp) holds its invariants,
also under ASan + UBSan; argument errors are raised before any native call."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import vfo_numpy as orc
from pyrayhf_amd import _native, library

import mp_vfo
import vfo_jacobian_numpy as vj

needs_mp = pytest.mark.skipif(not mp_vfo.available(), reason="mpmath is not installed: the 50-digit restatement cannot run")


def cases(g):
    for name in g["cases"]:
        name = str(name)
        yield name, {k: g[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt", "vh_mp", "jac_mp")}, \
            str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])


@pytest.fixture(scope="module")
def g26():
    return load_golden("g26_jacobian.npz")


def test_fixture_covers_the_cases_the_derivative_can_go_wrong_on(g26):
    seen = {"escape": 0, "n_points": set(), "modes": set(), "unmag": 0, "ragged": 0, "levels": set()}
    for name, c, mode, n_points in cases(g26):
        assert 4 <= c["freq"].size <= 6
        seen["escape"] += int(np.isnan(c["vh_mp"]).sum())
        seen["n_points"].add(n_points)
        seen["modes"].add(mode)
        seen["unmag"] += int(not c["bmag"].any())
        seen["ragged"] += int(np.ptp(np.diff(c["alt"])) > 1e-6)
        seen["levels"].add(c["den"].size)
        K = int(np.argmax(c["den"]))
        assert not c["jac_mp"][:, K:].any() and not c["jac_mp"][np.isnan(c["vh_mp"])].any()
    assert seen["escape"] and seen["n_points"] == {2, 63, 64, 65, 200} and seen["modes"] == {"O", "X"}
    assert seen["unmag"] and seen["ragged"] and seen["levels"] == {78, 620}
    assert 0.0 < float(g26["e_ref_O"]) < 1e-8 and 0.0 < float(g26["e_ref_X"]) < 1e-8


@needs_mp
def test_mp_values_match_the_oracle(g26):
    """1e-12 in X mode; 1e-6 - the project's O-mode parity bound, the oracle's own noise - in O mode; every pair."""
    for name, c, mode, n_points in cases(g26):
        mult = orc.stretch_multiplier(n_points)
        want = orc.virtual_heights(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, n_points)
        unmag = not c["bmag"].any()
        got = np.array([mp_vfo.virtual_height(f, c["den"], c["bmag"], c["bpsi"], c["alt"], mode, mult, unmag) for f in c["freq"]])
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got, c["vh_mp"], equal_nan=True), name          # what the generator stored
        ok = np.isfinite(want)
        rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
        assert rel.max() <= (1e-12 if mode == "X" else 1e-6), (name, rel.max())


def test_mp_jacobian_matches_differences_of_the_reference_in_x_mode(g26):
    """float64 central differences of the REFERENCE's vertical_forward_operator (relative step 1e-5, recorded by the
    generator) within 1e-6 of the row scale, on every entry where such a difference can be believed: the generator's
    ``fd_ok`` - steps 5e-5, 1e-5 and 2e-6 agree within 3e-7 and the difference is resolved in float64 - which holds for
    1050 of the 1086 bottomside entries of the reflecting X-mode rows (the rest: levels of negligible density, where the
    step is rounding noise, and the reflection level of frequencies next to foF2, where it is too long).  The
    two-point grid has no recorded differences (all noise: tools/gen_g26_jacobian.py)."""
    pinned = total = 0
    for name, c, mode, n_points in cases(g26):
        if mode != "X" or n_points == 2:
            continue
        fd, ok = g26[f"{name}_fd_ref"], g26[f"{name}_fd_ok"]
        K = int(np.argmax(c["den"]))
        for i in range(c["freq"].size):
            scale = np.abs(c["jac_mp"][i]).max()
            if scale == 0.0:
                assert not fd[i].any() and not ok[i].any(), (name, i)
                continue
            err = np.abs(fd[i] - c["jac_mp"][i])[ok[i]].max() / scale
            assert err <= 1e-6, (name, i, err)
            pinned += int(ok[i].sum())
            total += K
    assert total >= 1000 and pinned >= 0.9 * total, (pinned, total)


@needs_mp
def test_mp_jacobian_row_is_reproduced(g26):
    """One row of the fixture is computed again (the whole fixture takes the generator 14 s)."""
    name, c, mode, n_points = next(x for x in cases(g26) if x[0] == "c")
    i = 2
    vh, row = mp_vfo.jacobian_row(c["freq"][i], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, orc.stretch_multiplier(n_points))
    assert vh == c["vh_mp"][i] and np.array_equal(row, c["jac_mp"][i])


def test_numpy_restatement_reproduces_e_ref(g26):
    worst = {"O": 0.0, "X": 0.0}
    for name, c, mode, n_points in cases(g26):
        vh, J = vj.jacobian(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, orc.stretch_multiplier(n_points))
        assert np.array_equal(np.isnan(vh), np.isnan(c["vh_mp"])), name
        for i in range(c["freq"].size):
            scale = np.abs(c["jac_mp"][i]).max()
            if scale:
                worst[mode] = max(worst[mode], float(np.abs(J[i] - c["jac_mp"][i]).max() / scale))
            else:
                assert not J[i].any()
    for mode in "OX":
        assert worst[mode] <= float(g26[f"e_ref_{mode}"]) * (1 + 1e-12), (mode, worst)


# ---- header <-> binding ------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.load()
    for name, n_args in (("prhf_vfo_jacobian_f64", 17), ("prhf_vfo_vjp_f64", 18)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_native._PROTOTYPES[name][1]), name
        assert name in _native.exported_symbols() and hasattr(lib, name)
    assert "#define PRHF_ABI_VERSION 4" in text and _native.ABI_VERSION == 4
    for word in ("row of zeros", "k >= argmax den", "one-sided", "(1 - X)^(-1/2)"):
        assert word in text, word


def test_native_argument_errors_without_a_gpu():
    lib = _native.load()
    assert lib.prhf_vfo_jacobian_f64(None, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, None, 0) == _native.EINVAL
    assert b"context" in lib.prhf_last_error()
    assert lib.prhf_vfo_vjp_f64(None, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, None, None, 0) == _native.EINVAL


# ---- planner -----------------------------------------------------------------------------------------------------------
def _build_planner(tmp_path, extra):
    exe = tmp_path / "vjp_plan_host"
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", *extra, *inc, os.path.join(REPO, "tests", "devtools", "vjp_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("sanitize", [False, True])
def test_planner_invariants(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    exe = _build_planner(tmp_path, extra)
    run = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "vjp_plan_host: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    lines = {}
    for args in (("3", "5", "78", "0"), ("3", "5", "620", "1"), ("3", "5", "3000", "0"), ("1", "1", "620", "0")):
        lines[args] = subprocess.run([exe, "plan", *args], capture_output=True, text=True, timeout=60).stdout.strip()
    assert lines[("3", "5", "78", "0")] == "3 256 4 17152"
    assert lines[("3", "5", "620", "1")].startswith("3 256 4 ")
    assert lines[("3", "5", "3000", "0")].startswith("refused: the VJP stages at most ")
    assert lines[("1", "1", "620", "0")].split()[2] == "1"              # one frequency: one wave's rows


# ---- Python argument errors before any native call ---------------------------------------------------------------------
def test_argument_errors_are_raised_before_any_native_call(monkeypatch, g26):
    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    c = {k: g26[f"c_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt")}
    args = (c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"])
    g = np.ones(c["freq"].size)
    with pytest.raises(ValueError, match="mode must be 'O' or 'X'"):
        library.vertical_jacobian(*args, "Z", 50)
    with pytest.raises(ValueError, match="mode must be 'O' or 'X'"):
        library.vertical_vjp(*args, g, "Z", 50)
    with pytest.raises(ValueError, match="n_points"):
        library.vertical_jacobian(*args, "O", 0)
    with pytest.raises(ValueError):
        library.vertical_jacobian(c["freq"], c["den"][:5], c["bmag"], c["bpsi"], c["alt"], "O", 50)
    with pytest.raises(ValueError, match="alt must have one value per density level"):
        library.vertical_vjp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"][:5], g, "O", 50)
    with pytest.raises(ValueError, match="grad_vh must have the shape"):
        library.vertical_vjp(*args, g[:-1], "O", 50)
    with pytest.raises(ValueError, match="grad_vh must have the shape"):
        library.vertical_vjp(c["freq"], np.stack([c["den"]] * 2), c["bmag"], c["bpsi"], c["alt"], g, "O", 50)
    with pytest.raises(ValueError, match="freq must be a scalar or 1-D"):
        library.vertical_jacobian(c["freq"].reshape(1, -1, 1), c["den"], c["bmag"], c["bpsi"], c["alt"])
