"""Host-side checks of the JVP, no GPU: the new C symbol is declared, bound and exported and its
conventions documented; the launch planning (plan_jvp, jvp_chunk) holds its invariants, also under ASan + UBSan; argument
errors are raised before any native call; the float64 restatement's J @ t is inside the bound the GPU tests use."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import vfo_numpy as orc
from pyrayhf_amd import _native, fitting, library

import vfo_jacobian_numpy as vj


def test_the_symbol_is_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.load()
    m = re.search(r"\bint\s+prhf_vfo_jvp_f64\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m and len(m.group(1).split(",")) == 20 == len(_native._PROTOTYPES["prhf_vfo_jvp_f64"][1])
    assert "prhf_vfo_jvp_f64" in _native.exported_symbols() and hasattr(lib, "prhf_vfo_jvp_f64")
    for word in ("dvh = 0 for every tangent", "k >= argmax den are not read", "one-sided", "stages at most 1332 levels",
                 "n_tan == 0 is PRHF_OK"):
        assert word in text, word
    assert "vertical_jvp" in library.__all__ and "trace_sensitivity" in fitting.__all__


def test_native_argument_errors_without_a_gpu():
    lib = _native.load()
    assert lib.prhf_vfo_jvp_f64(None, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, 0, 0, None, None, 0) == _native.EINVAL
    assert b"context" in lib.prhf_last_error()


def _build_planner(tmp_path, extra):
    exe = tmp_path / "jvp_plan_host"
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", *extra, *inc, os.path.join(REPO, "tests", "devtools", "jvp_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("sanitize", [False, True])
def test_planner_invariants(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    exe = _build_planner(tmp_path, extra)
    run = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "jvp_plan_host: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr

    def plan(*args):
        return subprocess.run([exe, "plan", *args], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
    assert plan("3", "5", "78", "9") == ["3 512 5 8 2", "0 8 8 17152", "8 1 1 12784"]
    assert plan("3", "2", "620", "3") == ["3 256 2 4 1", "0 3 4 %d" % (621 * 96 + 620 * 16 + 2048 + 1280 + 4 * 620 * 8)]
    assert plan("3", "4", "1000", "11")[0] == "3 256 4 4 3"                     # past eight columns' room: four at a time
    assert plan("1", "1", "1332", "2")[0] == "1 256 1 1 2"
    assert plan("3", "5", "1333", "1")[0].startswith("refused: the JVP stages at most 1332 levels")


def test_argument_errors_are_raised_before_any_native_call(monkeypatch):
    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    g = load_golden("g26_jacobian.npz")
    c = {k: g[f"c_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt")}
    args = (c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"])
    with pytest.raises(ValueError, match="mode must be 'O' or 'X'"):
        library.vertical_jvp(*args, c["den"], "Z", 50)
    with pytest.raises(ValueError, match="tangents must have den's shape"):
        library.vertical_jvp(*args, c["den"][:-1], "O", 50)
    with pytest.raises(ValueError, match="tangents must have den's shape"):
        library.vertical_jvp(*args, np.ones((2, 3, c["den"].size)), "O", 50)
    with pytest.raises(ValueError, match="shared tangents must have shape"):
        library.vertical_jvp(*args, np.ones((2, 3, c["den"].size)), "O", 50, shared=True)
    with pytest.raises(ValueError, match="alt must have one value per density level"):
        library.vertical_jvp(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"][:5], c["den"], "O", 50)
    F2 = {"Nm": np.array([[[1e12]]]), "hm": np.array([[[300.0]]]), "B_bot": np.array([[[40.0]]])}
    with pytest.raises(ValueError, match="layer parameter 'B0'"):
        fitting.trace_sensitivity(F2, {}, {}, c["freq"], c["alt"], c["bmag"], c["bpsi"], ("NmF2", "B0"),
                                  edp_builder=lambda *a: c["den"])


def test_the_restatement_times_a_tangent_is_inside_the_gpu_tests_bound():
    """|J_numpy t - J_mp t| <= e_ref max_k |J_mp[f, :]| ||t||_1 by the definition of e_ref: a quarter of the bound
    tests/test_gpu_jvp.py holds the kernel to."""
    g = load_golden("g26_jacobian.npz")
    for name in ("c", "d", "g", "h"):
        c = {k: g[f"{name}_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt", "jac_mp")}
        mode, n_points = str(g[f"{name}_mode"]), int(g[f"{name}_n_points"])
        K = int(np.argmax(c["den"]))
        t = c["den"][None, :] * np.random.default_rng(26).uniform(-1.0, 1.0, size=(3, c["den"].size))
        J = vj.jacobian(c["freq"], c["den"], c["bmag"], c["bpsi"], c["alt"], mode, orc.stretch_multiplier(n_points))[1]
        diff = np.abs((J.astype(np.longdouble) - c["jac_mp"].astype(np.longdouble)) @ t.T.astype(np.longdouble)).astype(np.float64)
        bound = float(g[f"e_ref_{mode}"]) * (1 + 1e-12) * np.abs(c["jac_mp"]).max(axis=1)[:, None] * np.abs(t[:, :K]).sum(axis=1)[None, :]
        assert (diff <= bound).all(), name
