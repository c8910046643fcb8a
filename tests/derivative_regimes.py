"""Shared by tools/gen_g28_derivative_regimes.py and the tests of fixture g28 (TEST INFRASTRUCTURE ONLY): the bad-data
columns, the tall resampled columns, and the launch regime of a shape read from the host planning tools
(tests/devtools/vjp_plan_host.cpp, jvp_plan_host.cpp - the code prhf_api.cpp compiles; no LDS arithmetic here)."""

from __future__ import annotations

import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = ("freq", "den", "bmag", "bpsi", "alt", "vh_mp", "jac_mp")
BAD_COLUMNS = ("psimid", "psi0", "bmid", "btiny", "denmid", "denext")
N_UNIT = 24                      # unit tangents of a tall case: the JVP regime is planned for these


def kind_of(g, name):
    """tall, long or bad: the fixture's ``kinds`` runs parallel to its ``cases``."""
    return str(g["kinds"][[str(n) for n in g["cases"]].index(name)])


def bad_column(kind, den, bmag, bpsi, alt):
    """One bad-data variant of a clean column (copies).  K = argmax den of the clean column."""
    den, bmag, bpsi, alt = den.copy(), bmag.copy(), bpsi.copy(), alt.copy()
    K = int(np.argmax(den))
    if kind == "psimid":
        bpsi[K // 2] = np.nan
    elif kind == "psi0":
        bpsi[0] = np.nan
    elif kind == "bmid":                 # X mode: the running maximum of X + Y carries the NaN - an all-NaN trace
        bmag[K // 2] = np.nan
    elif kind == "btiny":                # nanmax|Y| < 1e-12: the isotropic branch in both modes, the NaN not counting
        bmag *= 1e-12
        bmag[K // 2] = np.nan
    elif kind == "denmid":               # np.argmax ranks the first NaN highest: the bottomside is cut there
        den[K // 2] = np.nan
    elif kind == "denext":               # ... or extended to there, peak included
        den[K + 3] = np.nan
    else:
        raise ValueError(kind)
    return den, bmag, bpsi, alt


def resample(alt, den, bmag, bpsi, n_alt, peak):
    """A column of n_alt levels, strictly increasing altitude, whose density peak is level `peak`: the levels below the
    source's peak spread over 0 ... peak, those above over the rest, values by linear interpolation and rounded to
    float32-representable doubles (they compress to half; the kernels see float64 either way)."""
    k = int(np.argmax(den))
    new = np.concatenate([np.linspace(alt[0], alt[k], peak + 1), np.linspace(alt[k], alt[-1], n_alt - peak)[1:]])
    new = new.astype(np.float32).astype(np.float64)
    out = [np.interp(new, alt, x).astype(np.float32).astype(np.float64) for x in (den, bmag, bpsi)]
    assert new.size == n_alt and (np.diff(new) > 0).all() and int(np.argmax(out[0])) == peak
    return new, out[0], out[1], out[2]


def highest_peak(den):
    """The library's rule for the levels to stage: np.argmax per profile, the first NaN ranking highest."""
    return int(max(int(np.argmax(d)) for d in np.atleast_2d(den)))


def build_tools(out_dir):
    """Compile the two planning tools; returns their paths."""
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]
    exes = {}
    for name in ("vjp_plan_host", "jvp_plan_host"):
        exe = os.path.join(str(out_dir), name)
        subprocess.run(["g++", "-std=c++17", "-O1", *inc, os.path.join(REPO, "tests", "devtools", name + ".cpp"), "-o", exe],
                       check=True)
        exes[name] = exe
    return exes


def _plan(exe, *args):
    return subprocess.run([exe, "plan", *map(str, args)], capture_output=True, text=True, timeout=60, check=True).stdout.strip()


def _staged(ask, n_alt, peak):
    """What the entry points do: plan for the whole column; where that is refused, for the levels up to the highest peak."""
    out = ask(n_alt)
    if not out.startswith("refused"):
        return n_alt, out
    return peak + 1, ask(peak + 1)


N_DENSE = 3                      # dense tangents of every case


def n_unit(kind, peak):
    """Unit tangents a case of this kind runs: 24 chosen levels on a tall column, every level below the peak elsewhere."""
    return N_UNIT if kind == "tall" else peak


def regime(exes, n_prof, n_freq, n_alt, peak, n_tan=N_UNIT):
    """[VJP waves, VJP lds_levels, Jacobian waves, Jacobian lds_levels, JVP chunk of the n_tan unit tangents, JVP
    lds_levels, JVP chunk of the three dense tangents]; waves / chunk 0: refused."""
    out = []
    for jac in (0, 1):
        levels, line = _staged(lambda L: _plan(exes["vjp_plan_host"], n_prof, n_freq, L, jac), n_alt, peak)
        out += [0 if line.startswith("refused") else int(line.split()[2]), levels]
    for count in (n_tan, N_DENSE):
        levels, text = _staged(lambda L: _plan(exes["jvp_plan_host"], n_prof, n_freq, L, count), n_alt, peak)
        chunk = 0 if text.startswith("refused") else int(text.splitlines()[0].split()[3])
        out += [chunk, levels] if count is n_tan and len(out) == 4 else [chunk]
    return np.array(out, dtype=np.int64)


def limits(exes):
    """(VJP, Jacobian, JVP) largest lds_levels, from the tools' refusal messages."""
    import re
    found = []
    for exe, last in ((exes["vjp_plan_host"], 0), (exes["vjp_plan_host"], 1), (exes["jvp_plan_host"], 1)):
        m = re.search(r"stages at most (\d+) levels", _plan(exe, 1, 1, 60000, last))
        found.append(int(m.group(1)))
    return tuple(found)
