#!/usr/bin/env python
"""Write tests/golden/g26_jacobian.npz: inputs, the 50-digit Jacobians of tests/mp_vfo.py, the error of the float64
restatement tests/vfo_jacobian_numpy.py against them (``e_ref`` per mode), and - X mode - central differences of the
REFERENCE's own vertical_forward_operator at a relative step of 1e-5.  Data only.

Build-container only (it imports the reference the way oracle/gen_golden.py does); takes about a minute.

Cases: seeded Chapman profiles thinned to 78 levels, one full 620-level profile, n_points in {2, 63, 64, 65, 200}, both
modes, an unmagnetised column, a non-uniform altitude grid.  Asserted below: some pair escapes, some reflects in the
first interval (j = 0), some has its bracket's running maximum attained below level j (an E-F valley), and no pair
sits within 1e-9 (relative) of a kink of the operator.
"""

from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import mp_vfo                                            # noqa: E402
import vfo_jacobian_numpy as vj                          # noqa: E402
from oracle import vfo_numpy as orc                      # noqa: E402
from oracle.gen_golden import load_reference_library     # noqa: E402
from pyrayhf_amd import synth                            # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g26_jacobian.npz")
KINK = 1e-9
FD_STEP = 1e-5


def bracket(f_mhz, den, bmag, alt, mode):
    """(reflects, j, jm, distance to the nearest kink of the reflection bracket) in float64."""
    K = int(np.argmax(den))
    f = f_mhz * 1e6
    c = orc.ratio_X(den[:K], f)
    if mode == "X":
        c = c + orc.ratio_Y(f, bmag[:K])
    r = np.maximum.accumulate(c)
    if not r[-1] >= 1.0:
        return False, -1, -1, abs(r[-1] - 1.0)
    if r[0] > 1.0:
        return True, -1, -1, abs(r[0] - 1.0)
    j = int(np.nonzero(r <= 1.0)[0][-1])
    jm = int(np.argmax(c[: j + 1]))
    others = np.delete(c[: j + 1], jm)
    tie = np.min(np.abs(others - c[jm]) / abs(c[jm])) if others.size else np.inf
    return True, j, jm, min(abs(r[j] - 1.0), abs(r[min(j + 1, K - 1)] - 1.0), tie)


def grid_kink(f_mhz, den, bmag, bpsi, alt, mode, n_points):
    """Smallest relative distance of a moving grid point to a level."""
    cols = orc.stretched_columns(np.array([f_mhz * 1e6]), den, bmag, bpsi, alt, mode, n_points)
    z = cols["alt"][0]
    if not np.isfinite(z).all():
        return np.inf
    K = int(np.argmax(den))
    m = orc.stretch_multiplier(n_points)
    moving = z[m > 0.0]
    return float(np.min(np.abs(moving[:, None] - alt[None, :K]) / np.abs(alt[None, :K])))


def frequencies(den, bmag, alt, mode, first_interval=True):
    """4-6 sounder frequencies [MHz] for one column: first interval (O mode), the valley when there is one, three
    ordinary reflections and one escape."""
    K = int(np.argmax(den))
    fn = orc.plasma_frequency(den[:K]) * 1e-6
    fo = fn.max()
    out = []
    if first_interval and mode == "O" and fn[1] > fn[0] > 0.0:
        out.append(float(np.sqrt(fn[0] * fn[1])))       # X_0 < 1 < X_1
    for eps in (0.004, 0.01, 0.02, 0.04, 0.08):         # just above a local maximum below the peak: the valley
        peaks = [k for k in range(1, K - 1) if fn[k] > fn[k - 1] and fn[k] > fn[k + 1]]
        found = False
        for k in peaks:
            f = fn[k] * (1.0 + eps) if mode == "O" else None
            if f is None:                               # X mode: the cutoff X + Y = 1 at that level, then a little above
                fh = orc.GYRO_CONST * bmag[k] * 1e-6
                f = (0.5 * (fh + np.sqrt(fh * fh + 4.0 * fn[k] ** 2))) * (1.0 + eps)
            ok, j, jm, _ = bracket(f, den, bmag, alt, mode)
            if ok and 0 <= jm < j:
                out.append(float(f))
                found = True
                break
        if found:
            break
    out += [float(0.55 * fo), float(0.8 * fo), float(0.97 * fo), float(1.4 * fo + 1.0)]
    return np.array(sorted(out))


def main():
    if not mp_vfo.available():
        raise SystemExit("mpmath is needed")
    lib = load_reference_library()
    alt620, den620, bmag620, bpsi620 = synth.chapman_profiles(40, 26)
    thin = slice(None, None, 8)
    alt78 = alt620[thin]
    k = np.arange(alt78.size)
    alt_nu = alt78 + 2.5 * np.sin(1.7 * k)
    # (name, profile row, levels, mode, n_points, variant)
    cases = [("a", 0, 78, "O", 2, ""), ("b", 0, 78, "X", 2, ""), ("c", 1, 78, "O", 63, ""), ("d", 1, 78, "X", 64, ""),
             ("e", 2, 78, "O", 65, ""), ("f", 2, 78, "X", 63, ""), ("g", 3, 78, "O", 200, ""), ("h", 3, 78, "X", 200, ""),
             ("i", 4, 78, "O", 64, ""), ("j", 4, 78, "X", 65, ""), ("k", 2, 78, "O", 64, "unmag"),
             ("l", 2, 78, "X", 63, "unmag"), ("m", 1, 78, "O", 63, "ragged"), ("n", 1, 78, "X", 65, "ragged"),
             ("o", 5, 620, "O", 65, ""), ("p", 5, 620, "X", 64, "")]
    out = {"cases": np.array([c[0] for c in cases])}
    e_ref = {"O": 0.0, "X": 0.0}
    seen = {"escape": 0, "first": 0, "valley": 0}
    fd_seen = [0, 0]
    for name, row, levels, mode, n_points, variant in cases:
        if levels == 78:
            alt, den, bmag, bpsi = alt78.copy(), den620[row, thin].copy(), bmag620[row, thin].copy(), bpsi620[row, thin].copy()
        else:
            alt, den, bmag, bpsi = alt620.copy(), den620[row].copy(), bmag620[row].copy(), bpsi620[row].copy()
        if variant == "unmag":
            bmag[:] = 0.0
        if variant == "ragged":
            alt = alt_nu.copy()
        K = int(np.argmax(den))
        second = np.max(np.delete(den, K))
        assert (den[K] - second) / den[K] > KINK, (name, "argmax tie")
        # (On a two-point grid the sum is little more than its last term, mu'(h - 1e-6) 1e-6.  For a pair that reflects in
        #  the first interval the reference's own O-mode value then moves by 3e-5 under 1-ulp jitter of its inputs
        #  (oracle noise_floor) - no value there can pin the 50-digit restatement to 1e-6; the first-interval pairs are
        #  the ones of the 63- to 200-point cases.)
        freq = frequencies(den, bmag, alt, mode, first_interval=n_points > 2)
        assert 4 <= freq.size <= 6, (name, freq)
        mult = orc.stretch_multiplier(n_points)
        unmag = variant == "unmag"
        vh_mp = np.empty(freq.size)
        J_mp = np.zeros((freq.size, den.size))
        for i, f in enumerate(freq):
            ok, j, jm, dist = bracket(f, den, bmag, alt, mode)
            assert dist > KINK, (name, f, "bracket kink", dist)
            assert grid_kink(f, den, bmag, bpsi, alt, mode, n_points) > KINK, (name, f, "grid point on a level")
            seen["escape"] += (not ok)
            seen["first"] += (ok and j == 0)
            seen["valley"] += (ok and 0 <= jm < j)
            vh_mp[i], J_mp[i] = mp_vfo.jacobian_row(f, den, bmag, bpsi, alt, mode, mult, unmag)
        vh_np, J_np = vj.jacobian(freq, den, bmag, bpsi, alt, mode, mult)
        vh_orc = orc.virtual_heights(freq, den, bmag, bpsi, alt, mode, n_points)
        assert np.array_equal(np.isnan(vh_mp), np.isnan(vh_orc)) and np.array_equal(np.isnan(vh_np), np.isnan(vh_orc)), name
        ok = np.isfinite(vh_orc)
        pin = np.abs(vh_mp[ok] - vh_orc[ok]) / np.abs(vh_orc[ok])
        assert pin.max() <= (1e-12 if mode == "X" else 1e-6), (name, "mp value against the oracle", pin)
        for i in range(freq.size):
            scale = np.abs(J_mp[i]).max()
            if scale > 0.0:
                e_ref[mode] = max(e_ref[mode], float(np.abs(J_np[i] - J_mp[i]).max() / scale))
            else:
                assert not J_np[i].any(), (name, i)
        out.update({f"{name}_freq": freq, f"{name}_den": den, f"{name}_bmag": bmag, f"{name}_bpsi": bpsi, f"{name}_alt": alt,
                    f"{name}_mode": np.array(mode), f"{name}_n_points": np.array(n_points), f"{name}_vh_mp": vh_mp,
                    f"{name}_jac_mp": J_mp})
        if mode == "X" and n_points > 2:
            # The reference's own operator, float64 central differences at a relative step of 1e-5 - and, to know where
            # such a difference can be believed at all, at 5e-5 and 2e-6 as well: an entry counts (fd_ok) where the three
            # agree within 3e-7 of their own row scale and the two evaluations differ by at least 2^-40 of the value (a
            # density of 0.01 m^-3 at level 0 does not move the float64 sum at all: three zeros agree; above 1e-3 of the peak
            # density an exact zero is believed).  Elsewhere the step 1e-5 is wrong for the entry, whatever the truth:
            # at a level whose density is 1e-6 of the peak's the absolute step is so small that the operator's float64
            # rounding is all the difference holds (level 0 of most columns: error growing as 1 / step), and next to the
            # reflection level of a frequency close to foF2 the step is too long (620 levels, 0.97 foF2: 2.4e-4, 1.9e-6,
            # 2.7e-8 of the row scale at steps 1e-4, 1e-5, 1e-6).
            # (Not on the two-point grid: there every difference is rounding noise of the float64 sum - 1.0e-6, 2.7e-6,
            # 1.4e-5, 1.4e-4 of the row scale at steps 1e-4 ... 1e-7 - while the analytic float64 row is within 2.4e-11 of
            # the 50-digit one.  The two-point rows are pinned by their values and by the analytic restatement.)
            fds, resolved = [], np.zeros((freq.size, den.size), dtype=bool)
            with np.errstate(all="ignore"):
                for rel in (FD_STEP, 5.0 * FD_STEP, 0.2 * FD_STEP):
                    fd = np.zeros((freq.size, den.size))
                    for kk in range(K):
                        step = rel * den[kk]
                        up, dn = den.copy(), den.copy()
                        up[kk] += step
                        dn[kk] -= step
                        hi = lib.vertical_forward_operator(freq, up, bmag, bpsi, alt, mode, n_points)
                        lo = lib.vertical_forward_operator(freq, dn, bmag, bpsi, alt, mode, n_points)
                        fd[:, kk] = (hi - lo) / (up[kk] - dn[kk])
                        if rel == FD_STEP:
                            # (a level above the reflection height changes nothing: an exact zero is its derivative)
                            resolved[:, kk] = (np.abs(hi - lo) >= 2.0 ** -40 * np.abs(vh_orc)) | \
                                              ((hi == lo) & (den[kk] >= 1e-3 * den[K]))
                    fd[~np.isfinite(vh_orc)] = 0.0
                    fds.append(fd)
            scale = np.abs(fds[0]).max(axis=1, keepdims=True)
            fd_ok = (np.abs(fds[1] - fds[0]) <= 3e-7 * scale) & (np.abs(fds[2] - fds[0]) <= 3e-7 * scale)
            fd_ok &= resolved
            fd_ok[:, K:] = False
            fd_ok[~np.isfinite(vh_orc)] = False
            out[f"{name}_fd_ref"] = fds[0]
            out[f"{name}_fd_ok"] = fd_ok
            for i in range(freq.size):
                sc = np.abs(J_mp[i]).max()
                if sc > 0.0:
                    err = np.abs(fds[0][i] - J_mp[i])[fd_ok[i]] / sc
                    fd_seen[0] += int(fd_ok[i].sum())
                    fd_seen[1] += K
                    assert err.max() <= 1e-6, (name, i, "differences of the reference", err.max())
                    print("   fd", name, i, "entries", int(fd_ok[i].sum()), "of", K, "worst", float(err.max()))
        print(name, mode, n_points, variant, "K", K, "freq", np.round(freq, 4), "e_ref so far", e_ref)
    assert seen["escape"] and seen["first"] and seen["valley"], seen
    assert fd_seen[0] >= 0.9 * fd_seen[1], fd_seen
    print("entries of X-mode rows pinned by differences of the reference:", fd_seen)
    out["e_ref_O"] = np.array(e_ref["O"])
    out["e_ref_X"] = np.array(e_ref["X"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", seen, e_ref)


if __name__ == "__main__":
    main()
