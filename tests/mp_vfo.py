"""A 50-digit mpmath restatement of the vertical forward operator for ONE (profile, frequency) pair, and its Jacobian
with respect to the density column by central differences (TEST INFRASTRUCTURE ONLY).

Restates reference ``PyRayHF/library.py:161-256`` (find_mu_mup), ``:324-438`` (regrid_to_nonuniform_grid) and
``:459-509`` (vertical_forward_operator) the way ``oracle/vfo_numpy.py`` does, with ``np.interp``'s bracket rule, but in
arithmetic whose rounding (1e-50) is far below anything float64 can see: its values are the truth the analytic
Jacobian of the operator is checked against (tools/gen_g26_jacobian.py, fixture tests/golden/g26_jacobian.npz).

Every float64 input is taken exactly (``mpf(float)``); the stretched grid ``m`` is the float64 array the operator uses.
"""

from __future__ import annotations

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
except ImportError:                                    # pragma: no cover - callers skip with a reason
    mpmath = None

DIGITS = 50
PLASMA_CONST = "8.97866275"
GYRO_CONST = "2.799249247e10"
BACKOFF = "1e-6"
UNMAG_TOL = 1e-12
REL_STEP = "1e-20"


def available():
    return mpmath is not None


def _setup():
    mp.dps = DIGITS


def _consts():
    # the reference's constants are float64 literals: take the float64 values exactly
    return mpf(float(PLASMA_CONST)), mpf(float(GYRO_CONST)), mpf(float(BACKOFF))


def unmagnetised(freq_mhz, den, bmag):
    """The isotropic decision of library.py:201 for one call: nanmax|Y| < 1e-12, a NaN |B| not counting (all NaN: False).
    |Y| is largest at the call's lowest frequency and, between levels, no larger than at a level."""
    K = int(np.argmax(np.asarray(den, dtype=np.float64)))
    b = np.abs(np.asarray(bmag, dtype=np.float64)[:K])
    b = b[~np.isnan(b)]
    if b.size == 0:
        return False
    f = float(np.min(np.abs(np.atleast_1d(np.asarray(freq_mhz, dtype=np.float64))))) * 1e6
    return bool(float(GYRO_CONST) * float(b.max()) / f < UNMAG_TOL)


def _interp(z, xp, fp):
    """np.interp for one abscissa: left / right clamps, x == xp[j] returns fp[j], bracket xp[j] <= z < xp[j+1]."""
    n = len(xp)
    if n == 1 or z <= xp[0]:
        return fp[0]
    if z >= xp[n - 1]:
        return fp[n - 1]
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if xp[mid] <= z:
            lo = mid
        else:
            hi = mid
    slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo])
    return slope * (z - xp[lo]) + fp[lo]


def _segment(z, xp):
    n = len(xp)
    if n == 1 or z <= xp[0]:
        return 0
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if xp[mid] <= z:
            lo = mid
        else:
            hi = mid
    return lo


def _mup(X, Y, psi_deg, mode, unmag):
    """mu' of library.py:161-256; None where the reference gives NaN."""
    if unmag:                                          # :201-207
        m2 = 1 - X
        if not m2 > 0:
            return None
        return 1 / mpmath.sqrt(m2)
    r = psi_deg * mpmath.pi / 180
    s, c = mpmath.sin(r), mpmath.cos(r)
    YT, YL = Y * s, Y * c
    Xm1 = 1 - X
    alpha = YT ** 4 / 4 + YL ** 2 * Xm1 ** 2
    beta = mpmath.sqrt(alpha)
    sign = 1 if mode == "O" else -1
    D = Xm1 - YT ** 2 / 2 + sign * beta
    if D == 0:
        return None
    rad = 1 - X * Xm1 / D
    if rad < 0:
        return None
    mu = mpmath.sqrt(rad)
    if mu > 1 or mu == 0:
        return None
    dbeta_dX = -YL ** 2 * Xm1 / beta
    dD_dX = -1 + sign * dbeta_dX
    dalpha_dY = YT ** 3 * s + 2 * YL * Xm1 ** 2 * c
    dbeta_dY = dalpha_dY / (2 * beta)
    dD_dY = -YT * s + sign * dbeta_dY
    dmu_dY = (X * Xm1 * dD_dY) / (2 * mu * D ** 2)
    dmu_dX = (1 / (2 * mu * D)) * (2 * X - 1 + X * Xm1 / D * dD_dX)
    mup = mu - (2 * X * dmu_dX + Y * dmu_dY)
    return None if mpmath.isnan(mup) else mup              # a NaN |B| or psi: the term is skipped by nansum (:288)


class Pair:
    """One (profile, frequency, mode, grid): the operator's value and, by differences, its Jacobian row."""

    def __init__(self, freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag=None):
        _setup()
        self.kp, self.kg, self.backoff = _consts()
        den = np.asarray(den, dtype=np.float64)
        self.K = int(np.argmax(den))                   # :371-375
        self.n_alt = den.size
        K = self.K
        self.f = mpf(float(freq_mhz)) * mpf(10) ** 6
        self.den = [mpf(float(v)) for v in den[:K]]
        self.b = [mpf(float(v)) for v in np.asarray(bmag)[:K]]
        self.p = [mpf(float(v)) for v in np.asarray(bpsi)[:K]]
        self.a = [mpf(float(v)) for v in np.asarray(alt)[:K]]
        self.alt_min = mpf(float(np.min(alt)))
        self.m = [mpf(float(v)) for v in np.asarray(mult, dtype=np.float64)]
        self.mode = mode
        if unmag is None:
            # :201 - nanmax|Y| over the call's array; callers with several frequencies pass the call-wide answer
            unmag = unmagnetised(freq_mhz, den, bmag)
        self.unmag = bool(unmag)

    # -- reflection ----------------------------------------------------------------------
    def _cond(self, den):
        f2 = self.f * self.f
        out = []
        for k in range(self.K):
            X = (mpmath.sqrt(den[k]) * self.kp) ** 2 / f2
            out.append(X if self.mode == "O" else X + self.kg * self.b[k] / self.f)
        return out

    def bracket(self, den=None):
        """(reflects, j, jm, r_j, r_j1): np.interp's bracket of 1.0 in the running maximum, and the level jm <= j where
        that running maximum was attained first.  j = -1: left clamp; j = K - 1: the last level is hit exactly."""
        c = self._cond(self.den if den is None else den)
        if any(mpmath.isnan(v) for v in c):            # np.maximum.accumulate carries a NaN to the last level: no reflection
            return False, None, None, None, None
        run, arg, best, bi = [], [], None, -1
        for k, v in enumerate(c):
            if best is None or v > best:
                best, bi = v, k
            run.append(best)
            arg.append(bi)
        if not run or run[-1] < 1:
            return False, None, None, None, None
        if run[0] >= 1 and (self.K == 1 or run[0] > 1):
            return True, -1, -1, None, run[0]
        j = max(k for k in range(self.K) if run[k] <= 1)
        if j == self.K - 1:
            return True, j, arg[j], run[j], None
        return True, j, arg[j], run[j], run[j + 1]

    def height(self, den=None):
        if mpmath.isnan(self.alt_min):                 # min(alt) is added to every sum (:292): no pair has a value
            return None
        ok, j, _, rj, rj1 = self.bracket(den)
        if not ok:
            return None
        if j == -1:
            h = self.a[0]
        elif rj1 is None or rj == 1:
            h = self.a[j]
        else:
            h = (self.a[j + 1] - self.a[j]) / (rj1 - rj) * (1 - rj) + self.a[j]
        return h - self.backoff                        # :407

    # -- the sum -------------------------------------------------------------------------
    def _terms(self, den, h, only=None):
        """Per grid point: mu' * thickness (None where NaN) and the np.interp segment of the point."""
        n = len(self.m)
        H = h - self.a[0]
        z = [self.m[i] * H + self.a[0] for i in range(n)]
        f2 = self.f * self.f
        terms, segs = [None] * n, [0] * n
        for i in range(n):
            segs[i] = _segment(z[i], self.a)
            if only is not None and segs[i] not in only:
                continue
            d = _interp(z[i], self.a, den)
            X = (mpmath.sqrt(d) * self.kp) ** 2 / f2
            Y = self.kg * _interp(z[i], self.a, self.b) / self.f
            psi = _interp(z[i], self.a, self.p)
            mup = _mup(X, Y, psi, self.mode, self.unmag)
            dist = (z[i + 1] - z[i]) if i + 1 < n else self.backoff
            terms[i] = None if mup is None else mup * dist
        return terms, segs

    def value(self):
        """Virtual height [km] or None (NaN)."""
        h = self.height()
        if h is None:
            return None
        terms, _ = self._terms(self.den, h)
        total = sum((t for t in terms if t is not None), mpf(0))
        return None if total == 0 else total + self.alt_min

    def jacobian_row(self):
        """d vh / d den_k for every level of the column (zeros at and above the peak, a zero row for a NaN value), by
        central differences with a relative step of 1e-20; also returns the value.  A level outside the reflection
        bracket only moves the grid points of its two segments, so only those are evaluated again."""
        row = [mpf(0)] * self.n_alt
        h = self.height()
        if h is None:
            return None, row
        base, segs = self._terms(self.den, h)
        total = sum((t for t in base if t is not None), mpf(0))
        if total == 0:
            return None, row
        _, j, jm, _, _ = self.bracket()
        moves_h = {jm, j + 1} if j >= 0 and j + 1 < self.K else set()
        step = mpf(REL_STEP)
        for k in range(self.K):
            dk = self.den[k] * step if self.den[k] != 0 else step
            vals = []
            for sgn in (1, -1):
                den = list(self.den)
                den[k] = den[k] + sgn * dk
                if k in moves_h:
                    hk = self.height(den)
                    t, _ = self._terms(den, hk)
                    vals.append(sum((x for x in t if x is not None), mpf(0)))
                else:
                    only = {k - 1, k}
                    t, _ = self._terms(den, h, only)
                    vals.append(sum((t[i] - base[i] for i in range(len(t))
                                     if segs[i] in only and t[i] is not None and base[i] is not None), mpf(0)))
            row[k] = (vals[0] - vals[1]) / (2 * dk)
        return total + self.alt_min, row


def virtual_height(freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag=None):
    """float64 of the 50-digit value (NaN where the reference gives NaN)."""
    v = Pair(freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag).value()
    return float("nan") if v is None else float(v)


def jacobian_row(freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag=None):
    """(vh, row) as float64: the 50-digit value and Jacobian row, rounded once at the end."""
    v, row = Pair(freq_mhz, den, bmag, bpsi, alt, mode, mult, unmag).jacobian_row()
    return (float("nan") if v is None else float(v)), np.array([float(x) for x in row])
