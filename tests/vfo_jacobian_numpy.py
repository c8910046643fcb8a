"""float64 NumPy restatement of the ANALYTIC Jacobian d vh / d den of the vertical forward operator (TEST
INFRASTRUCTURE ONLY; DESIGN.md section 4.14 has the derivation).

The function differentiated is the discrete sum of ``oracle/vfo_numpy.virtual_heights``.  Its error against the 50-digit
truth of ``tests/mp_vfo.py`` is what float64 can do for this derivative (fixture g26, ``e_ref``), and the GPU kernels
are held to 4 x that.  The group index is evaluated around a = 1 - X (no cancellation at reflection) and carried with
two tangents by forward-mode dual numbers: d/dX, and d/dz along the segment through Y and psi.
"""

from __future__ import annotations

import numpy as np

PLASMA_CONST = 8.97866275
GYRO_CONST = 2.799249247e10
BACKOFF = 1e-6
UNMAG_TOL = 1e-12
DEG = 0.017453292519943295


def unmagnetised(freq_mhz, bottom_bmag):
    """nanmax|Y| < 1e-12 over the call (library.py:201): a NaN |B| does not count; all NaN: magnetised."""
    b = np.abs(np.asarray(bottom_bmag, dtype=np.float64))
    b = b[~np.isnan(b)]
    if b.size == 0:
        return False
    return bool(GYRO_CONST * b.max() / (np.min(np.abs(np.atleast_1d(freq_mhz))) * 1e6) < UNMAG_TOL)


class Dual:
    """value + two tangents, elementwise on arrays."""

    __slots__ = ("v", "a", "b")

    def __init__(self, v, a=0.0, b=0.0):
        self.v, self.a, self.b = v, a, b

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(x)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, self.a + o.a, self.b + o.b)

    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o)
        return Dual(self.v - o.v, self.a - o.a, self.b - o.b)

    def __rsub__(self, o):
        return Dual.lift(o) - self

    def __neg__(self):
        return Dual(-self.v, -self.a, -self.b)

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, self.a * o.v + self.v * o.a, self.b * o.v + self.v * o.b)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.v / o.v
        return Dual(q, (self.a - q * o.a) / o.v, (self.b - q * o.b) / o.v)

    def __rtruediv__(self, o):
        return Dual.lift(o) / self

    def sqrt(self):
        r = np.sqrt(self.v)
        return Dual(r, self.a / (2.0 * r), self.b / (2.0 * r))


def group_index_dual(X, Y2, S2, C2, mode):
    """mu' (Dual) from Dual X, Y^2, sin^2 psi, cos^2 psi below the reflection height, around a = 1 - X:
    h = Y_T^2/2, t = Y_L^2 a, beta = sqrt(h^2 + t a), G = s beta - h (O mode: t a / (beta + h), no cancellation),
    D = a + G, N = G + a^2, w = 1/sqrt(N D), q = 1 - (N w)^2, mu' = w [q (1 + s t (1 + X) / (2 beta)) + D - X]."""
    a = 1.0 - X
    YL2 = Y2 * C2
    h = 0.5 * (Y2 * S2)
    t = YL2 * a
    ta = t * a
    beta = (h * h + ta).sqrt()
    if mode == "O":
        G = ta / (beta + h)
        sgn = 1.0
    else:
        G = -(beta + h)
        sgn = -1.0
    D = a + G
    N = G + a * a
    w = 1.0 / (N * D).sqrt()
    v = t * (1.0 - 0.5 * a)
    Sp1 = 1.0 + sgn * (v / beta)
    Nw = N * w
    q = 1.0 - Nw * Nw
    U = Sp1 * q + (D - X)
    mup = w * U
    # (mu^2 = N / D > 1 exactly where X > 1 - a grid collapsed onto a level above the cutoff, below the gyrofrequency:
    #  library.py:238 makes the term NaN)
    ok = (D.v > 0.0) & (N.v * D.v > 0.0) & (a.v >= 0.0)
    return mup, ok


def jacobian_row(freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag=None):
    """(vh, row (n_alt,)): the analytic derivative of the discrete sum for one pair.  A pair without a value - whatever
    made vh NaN, min(alt) included - has a row of (finite) zeros."""
    den, bmag, bpsi, alt = (np.asarray(x, dtype=np.float64) for x in (den, bmag, bpsi, alt))
    m = np.asarray(mult, dtype=np.float64)
    n_alt, n = den.size, m.size
    row = np.zeros(n_alt)
    K = int(np.argmax(den))
    if K == 0:
        return np.nan, row
    d, b, p, a = den[:K], bmag[:K], bpsi[:K], alt[:K]
    f = float(freq_mhz) * 1e6
    f2 = f * f
    cX = (PLASMA_CONST * PLASMA_CONST) / f2
    cY = GYRO_CONST / f
    if unmag is None:
        unmag = unmagnetised(freq_mhz, b)
    with np.errstate(all="ignore"):
        fn = np.sqrt(d) * PLASMA_CONST
        c = (fn * fn) / f2
        if mode == "X":
            c = c + (GYRO_CONST * b) / f
        r = np.maximum.accumulate(c)
        if not r[-1] >= 1.0:
            return np.nan, row
        # np.interp's bracket and the derivative of the reflection height
        Hk = np.zeros(K)
        if r[0] > 1.0 or K == 1:
            h = a[0]
        else:
            j = int(np.nonzero(r <= 1.0)[0][-1])
            if j == K - 1 or r[j] == 1.0:
                h = a[j]
            else:
                da, dr = a[j + 1] - a[j], r[j + 1] - r[j]
                h = (da / dr) * (1.0 - r[j]) + a[j]
                jm = int(np.argmax(c[: j + 1]))                     # first level that attains the running maximum
                Hk[jm] += -da * (r[j + 1] - 1.0) / (dr * dr) * cX
                Hk[j + 1] += -da * (1.0 - r[j]) / (dr * dr) * cX
        h = h - BACKOFF
        H = h - a[0]
        z = m * H + a[0]
        dist = np.append(np.diff(z), BACKOFF)
        wgt = np.append(np.diff(m), 0.0)
        # np.interp segment and abscissa of every grid point (clamped below level 0)
        s = np.clip(np.searchsorted(a, z, side="right") - 1, 0, max(K - 2, 0))
        dz = np.where(z > a[0], z - a[s], 0.0)
        if K > 1:
            seg_len = a[s + 1] - a[s]
            sden = np.where(dz > 0.0, (d[s + 1] - d[s]) / seg_len, 0.0)
            sb = np.where(dz > 0.0, (b[s + 1] - b[s]) / seg_len, 0.0)
            sp = np.where(dz > 0.0, (p[s + 1] - p[s]) / seg_len, 0.0)
            tt = dz / seg_len
        else:
            sden = sb = sp = tt = np.zeros(n)
        den_i = sden * dz + d[s]
        X = Dual(cX * den_i, 1.0, 0.0)
        if unmag:
            am = 1.0 - X
            mup = 1.0 / am.sqrt()
            ok = am.v > 0.0
        else:
            Y = cY * (sb * dz + b[s])
            psi = (sp * dz + p[s]) * DEG
            sn, cs = np.sin(psi), np.cos(psi)
            s2p = 2.0 * (sn * cs) * (sp * DEG)
            Y2 = Dual(Y * Y, 0.0, 2.0 * Y * (cY * sb))
            S2 = Dual(sn * sn, 0.0, s2p)
            C2 = Dual(cs * cs, 0.0, -s2p)
            mup, ok = group_index_dual(X, Y2, S2, C2, mode)
        ok = ok & np.isfinite(mup.v) & np.isfinite(mup.a) & np.isfinite(mup.b)
        term = np.where(ok, mup.v * dist, 0.0)
        total = term.sum()
        if total == 0.0:
            return np.nan, row
        GX = np.where(ok, dist * mup.a * cX, 0.0)
        SH = np.where(ok, mup.v * wgt, 0.0).sum() + np.where(ok, dist * m * mup.b, 0.0).sum()
        # the total dX of every node per level before it meets d mu'/dX: interpolation weights + the node's own motion
        dX = np.zeros((n, K))
        idx = np.arange(n)
        dX[idx, s] += 1.0 - tt
        if K > 1:
            dX[idx, s + 1] += tt
        dX += np.outer(m * sden, Hk)
        vh = total + np.min(alt)
        if not np.isfinite(vh):                                         # (a NaN altitude)
            return np.nan, row
        row[:K] = (GX[:, None] * dX).sum(axis=0) + SH * Hk
    return vh, row


def jacobian(freq_mhz, den, bmag, bpsi, alt, mode, mult):
    """(vh (F,), J (F, n_alt)) for one profile; the isotropic branch is decided for the call, as the reference does."""
    freq = np.atleast_1d(np.asarray(freq_mhz, dtype=np.float64))
    K = int(np.argmax(den))
    unmag = unmagnetised(freq, np.asarray(bmag)[:K]) if K else True
    vh = np.empty(freq.size)
    J = np.zeros((freq.size, np.asarray(den).size))
    for i, fm in enumerate(freq):
        vh[i], J[i] = jacobian_row(fm, den, bmag, bpsi, alt, mode, mult, unmag)
    return vh, J
