"""The launches whose bits tests/golden/g27_panel_bits.npz records (tools/gen_golden_panel_bits.py writes it,
tests/test_gpu_panel_pipeline.py compares with it): every shape at which the panel block of lean_loop_body takes
another path.  Inputs come from the seeds of the helpers named below, so the fixture holds outputs and counters only.

  b<n>_p<4|8>     24 x 48 pairs, X mode, n = 8192, 8200, 20000 points, panel_nodes = 4 and 8: several lists per pair,
                  the general list, a region end that is no multiple of the block
  long65535       24 x 8 pairs at 65535 points: lists of more than 64 entries (the second list register), runs near the
                  cap of 128 entries
  plateau<n>      rows 5-9 of plateau_inputs at 8192 and 20000 points: pairs that fall back and pairs that keep the lower
                  region (a list made a second time)
  omode, nonuniform, n4096    launches the panel sum must not touch

A case is (virtual heights, panel_counters' increase, panel_upper_counters' increase)."""

import numpy as np

from test_gpu_panel_sum import FREQ, SIZES, grid
from test_strided_sum_host import plateau_inputs

SEED = 20261019


def make_context(**options):
    from pyrayhf_amd import _native
    ctx = _native.Context(0)
    ctx.set_option("target_waves", 64)
    for name, value in options.items():
        ctx.set_option(name, value)
    return ctx


def launch(ctx, freq, den, bmag, bpsi, alt, n_points, mode="X"):
    """test_gpu_panel_sum.run, with both pairs of counters."""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points)
    out = np.full((d.shape[0], f.size), -7.0)
    before = ctx.panel_counters() + ctx.panel_upper_counters()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    after = ctx.panel_counters() + ctx.panel_upper_counters()
    return out, np.array([x - y for x, y in zip(after, before)], dtype=np.int64)


def inputs():
    """{case: (panel_nodes, launch's arguments, keywords)}"""
    from conftest import load_golden
    from pyrayhf_amd import synth
    alt, den, bmag, bpsi = synth.chapman_profiles(24, SEED)
    pf, palt, pden, pbmag, pbpsi = plateau_inputs()
    g = load_golden("g7_edges.npz")
    nfreq, nden, nbmag, nbpsi, nalt = (g[f"nonuniform_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt"))
    tile = lambda x: np.tile(x, (24, 1))                   # noqa: E731
    cases = {}
    for n in SIZES:
        for nodes in (4, 8):
            cases[f"b{n}_p{nodes}"] = (nodes, (FREQ, den, bmag, bpsi, alt, n), {})
    cases["long65535"] = (4, (FREQ[::6], den, bmag, bpsi, alt, 65535), {})
    for n in (8192, 20000):
        cases[f"plateau{n}"] = (4, (pf, pden[5:10], pbmag[5:10], pbpsi[5:10], palt, n), {})
    cases["omode"] = (4, (FREQ, den, bmag, bpsi, alt, 8192), {"mode": "O"})
    cases["nonuniform"] = (4, (nfreq, tile(nden), tile(nbmag), tile(nbpsi), nalt, 8192), {})
    cases["n4096"] = (4, (FREQ, den, bmag, bpsi, alt, 4096), {})
    return cases


UNTOUCHED = ("omode", "nonuniform", "n4096")


def hipcc_version_line():
    """The compiler line that names the build: the same source gives the same bits only under the same compiler.
    It is the installed compiler's, which is the library's only if the library was built here and now (build() does);
    `unknown` where no hipcc is found."""
    import subprocess
    try:
        text = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return "unknown"
    lines = [ln.strip() for ln in text.splitlines() if "clang version" in ln or "HIP version" in ln]
    return " | ".join(lines) if lines else "unknown"
