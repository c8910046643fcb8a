"""The un-fused stage functions of the path as standalone device ops, against the reference's
stage captures (fixture G6, reference regrid_to_nonuniform_grid / find_X / find_Y / find_mu_mup /
find_vh run on the Day profile) and its structural tests."""

import math

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import LIMIT_CAP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pyrayhf_amd import library
    return library


@pytest.mark.parametrize("mode", ["O", "X"])
def test_regrid_is_bit_identical_to_the_reference(lib, mode):
    g = load_golden("g4_day_night.npz")
    s = load_golden("g6_stages.npz")
    rg = lib.regrid_to_nonuniform_grid(s["freq"] * 1e6, g["Day_den"], g["Day_bmag"], g["Day_bpsi"], g["Day_alt"],
                                       mode=mode, n_points=50)
    assert set(rg) == {"freq", "den", "bmag", "bpsi", "dist", "alt", "crit_height", "ind"}   # library.py:430-437
    for key in ("den", "bmag", "bpsi", "dist", "alt", "crit_height"):
        assert rg[key].shape == (3, 50)
        assert same_bits(rg[key], s[f"{mode}_{key}"]), key
    assert np.array_equal(rg["freq"], np.repeat(s["freq"][:, None] * 1e6, 50, axis=1))
    assert rg["ind"].dtype == np.int64 and np.array_equal(rg["ind"], np.tile(np.arange(50), (3, 1)))


def test_regrid_basic_structure_and_escaping_rows(lib):
    # reference test_core.py:191-207
    f = np.array([1.0e6, 2.0e6, 2.0e7])
    rg = lib.regrid_to_nonuniform_grid(f, np.array([1.0e11, 5.0e11, 1.0e12]), np.full(3, 5.0e-5), np.full(3, 60.0),
                                       np.array([100, 200, 300]), mode="O", n_points=10)
    assert isinstance(rg, dict) and rg["freq"].shape[0] == len(f) and rg["den"].shape[0] == len(f)
    # 20 MHz escapes: NaN altitudes, but the last thickness is still the 1e-6 km back-off (library.py:415-416)
    assert np.all(np.isnan(rg["alt"][2])) and np.all(np.isnan(rg["dist"][2, :-1])) and rg["dist"][2, -1] == 1e-6
    assert np.all(np.isnan(rg["crit_height"][2]))
    with pytest.raises(ValueError, match="mode must be 'O' or 'X'"):
        lib.regrid_to_nonuniform_grid(f, np.ones(3), np.ones(3), np.ones(3), np.arange(3.0), mode="Q")


@pytest.mark.parametrize("mode", ["O", "X"])
def test_find_vh_on_stage_captures(lib, mode):
    g = load_golden("g4_day_night.npz")
    s = load_golden("g6_stages.npz")
    vh = lib.find_vh(s[f"{mode}_X"], s[f"{mode}_Y"], s[f"{mode}_bpsi"], s[f"{mode}_dist"],
                     float(np.min(g["Day_alt"])), mode)
    assert vh.shape == (3,)
    np.testing.assert_allclose(vh, s[f"{mode}_vh"], rtol=1e-6 if mode == "O" else 1e-11)


def test_find_vh_small_known_answer(lib):
    # reference test_core.py:155-168 (+ the value the reference returns for it)
    k = load_golden("g3_index_kat.npz")
    vh = lib.find_vh(np.array([[0.5, 0.6]]), np.array([[0.1, 0.2]]), np.array([[45.0, 45.0]]),
                     np.array([[1.0, 1.0]]), 100.0, "O")
    assert isinstance(vh, np.ndarray) and vh.shape == (1,) and vh[0] > 100.0
    np.testing.assert_allclose(vh, k["find_vh_small"], rtol=1e-13)
    # every term NaN -> exact zero -> NaN (library.py:290)
    assert np.isnan(lib.find_vh(np.array([[1.5, 2.0]]), np.array([[0.1, 0.2]]), np.array([[45.0, 45.0]]),
                                np.array([[1.0, 1.0]]), 100.0, "O")[0])


def test_unfused_chain_equals_fused_operator(lib):
    """regrid -> find_X / find_Y -> find_vh (the reference's own composition, library.py:495-507)
    against the fused kernel on the same profile."""
    g = load_golden("g4_day_night.npz")
    freq = g["freq"][20:120:7]
    args = (g["Night_den"], g["Night_bmag"], g["Night_bpsi"], g["Night_alt"])
    for mode, n in (("X", 400), ("O", 200)):
        rg = lib.regrid_to_nonuniform_grid(freq * 1e6, *args, mode=mode, n_points=n)
        with np.errstate(all="ignore"):
            X = lib.find_X(rg["den"], rg["freq"])
            Y = lib.find_Y(rg["freq"], rg["bmag"])
        chain = lib.find_vh(X, Y, rg["bpsi"], rg["dist"], float(np.min(g["Night_alt"])), mode)
        fused = lib.vertical_forward_operator(freq, *args, mode, n, math=lib.MATH_FAITHFUL)
        assert np.array_equal(np.isnan(chain), np.isnan(fused))
        ok = np.isfinite(fused)
        np.testing.assert_allclose(chain[ok], fused[ok], rtol=1e-12 if mode == "X" else 2e-5)


# ----------------------------------------------------------------------------------------------------------------
# Every code path of the three stage ops: mu_mup_kernel's two-trip and remainder loops, the 16-byte
# and scalar paths and the odd-element tail, the whole-array isotropic test, find_vh's row shapes, and regrid on
# grids, columns and edges the reference fixtures G6 / G16 and the oracle cover.  Device-pointer calls go through the
# context the way bench.py makes them, on torch tensors; every output starts as SENTINEL so that an element never
# written shows up.
# ----------------------------------------------------------------------------------------------------------------
SENTINEL = -1.2345678e300
PERIOD = 4099                    # prime: the tiled triples never line up with a workgroup's piece or a wavefront
TIERS = {"faithful": 0, "fast": 1}
MU_SIZES = [1, 2, 3, 255, 256, 257, 511, 513, 2_097_151, 2_097_152, 2_097_154, 2_098_177, 6_291_459]


def _triples(n, seed):
    """n distinct-ish (X, Y, psi) triples: both sides of X = 1 and of Y = 1, every quadrant of psi."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.4, n)
    Y = rng.uniform(0.0, 1.4, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    P = rng.uniform(-90.0, 270.0, n)
    return X, Y, P


def _on_device(a, offset):
    """a as a float64 CUDA tensor view starting `offset` elements into its storage (offset 1: 8-byte aligned only)."""
    import torch
    t = torch.empty(a.size + offset, dtype=torch.float64, device="cuda")
    t[offset:] = torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")      # (a writable copy)
    return t[offset:]


def _sentinel_like(n, offset):
    import torch
    return torch.full((n + offset,), SENTINEL, dtype=torch.float64, device="cuda")[offset:]


def _mu_mup(lib, X, Y, P, mode, tier, placement):
    """find_mu_mup through the host wrapper (placement "host") or on device pointers at storage offset 0 / 1."""
    from pyrayhf_amd import _native
    if placement == "host":
        return lib.find_mu_mup(X, Y, P, mode, math=tier)
    import torch
    off = {"aligned": 0, "offset1": 1}[placement]
    x, y, p = (_on_device(a, off) for a in (X, Y, P))
    mu, mup = _sentinel_like(X.size, off), _sentinel_like(X.size, off)
    if off == 0:
        assert all(t.data_ptr() % 16 == 0 for t in (x, y, p, mu, mup))
    else:
        assert all(t.data_ptr() % 16 == 8 for t in (x, y, p, mu, mup))
    torch.cuda.synchronize()
    ctx = _native.host_context()
    ctx.set_math(tier)
    _native.raise_for(ctx.mu_mup(x.data_ptr(), y.data_ptr(), p.data_ptr(), X.size, lib._MODE_CODE[mode],
                                 mu.data_ptr(), mup.data_ptr(), _native.FLAG_DEVICE_PTRS))
    return mu.cpu().numpy(), mup.cpu().numpy()


def _find_vh(lib, X, Y, P, D, alt_min, mode, tier, placement):
    from pyrayhf_amd import _native
    if placement == "host":
        return lib.find_vh(X, Y, P, D, alt_min, mode, math=tier)
    import torch
    rows, cols = X.shape
    if placement == "aligned":
        flat = [_on_device(a.reshape(-1), 0) for a in (X, Y, P, D)]
        ptrs = [t.data_ptr() for t in flat]
        assert all(q % 16 == 0 for q in ptrs)          # (even n_cols: every row on the 16-byte path)
        stride = cols
    else:
        # every row starts at an odd element offset (8 bytes past a 16-byte boundary): one element in front and an
        # even row stride (odd n_cols: one NaN of padding per row, which is never read)
        stride = cols if cols % 2 == 0 else cols + 1
        flat = []
        for a in (X, Y, P, D):
            pad = np.full((rows, stride), np.nan)
            pad[:, :cols] = a
            flat.append(_on_device(pad.reshape(-1), 1))
        ptrs = [t.data_ptr() for t in flat]
    vh = _sentinel_like(rows, 0)
    torch.cuda.synchronize()
    ctx = _native.host_context()
    ctx.set_math(tier)
    if stride == cols:
        assert all(q % 16 == 8 for q in ptrs) or placement == "aligned"
        _native.raise_for(ctx.find_vh(*ptrs, rows, cols, alt_min, lib._MODE_CODE[mode], vh.data_ptr(),
                                      _native.FLAG_DEVICE_PTRS))
        return vh.cpu().numpy()
    # (the ABI takes contiguous rows: a padded row is one call per row, each at its own odd offset)
    out = np.empty(rows)
    for r in range(rows):
        one = _sentinel_like(1, 0)
        torch.cuda.synchronize()
        assert (ptrs[0] + 8 * r * stride) % 16 == 8
        _native.raise_for(ctx.find_vh(*(q + 8 * r * stride for q in ptrs), 1, cols, alt_min, lib._MODE_CODE[mode],
                                      one.data_ptr(), _native.FLAG_DEVICE_PTRS))
        out[r] = one.cpu().numpy()[0]
    return out


_tiled = {}


def _tiled_inputs(n):
    if n not in _tiled:
        _tiled.clear()
        X, Y, P = _triples(PERIOD, 1701)
        _tiled[n] = tuple(np.resize(a, n) for a in (X, Y, P))
    return _tiled[n]


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("mode", ["O", "X"])
@pytest.mark.parametrize("n", MU_SIZES)
def test_mu_mup_every_loop_and_placement_bit_for_bit(lib, n, mode, tier):
    """Sizes around the 256-thread workgroup, the 4096-workgroup grid cap (n > 2^21: the two-trip loop and its
    remainder) and the odd tail; host, 16-byte-aligned and 8-byte-aligned device arrays.  Each element must equal,
    bit for bit, the result of the same triple in a small host call: a misindexed load or store, or an element that
    is skipped, fails; and alignment changes no bit (every path runs the same per-element arithmetic)."""
    level = TIERS[tier]
    X0, Y0, P0 = _triples(PERIOD, 1701)
    mu0, mup0 = lib.find_mu_mup(X0, Y0, P0, mode, math=level)
    X, Y, P = (a[:n] for a in (X0, Y0, P0)) if n <= PERIOD else _tiled_inputs(n)
    want_mu, want_mup = np.resize(mu0, n), np.resize(mup0, n)
    for placement in ("host", "aligned", "offset1"):
        mu, mup = _mu_mup(lib, X, Y, P, mode, level, placement)
        for got, want, name in ((mu, want_mu, "mu"), (mup, want_mup, "mup")):
            bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
            assert not bad.any(), (placement, name, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


def _index_reference(X, Y, P, mode, runs=24):
    """The oracle's mu, mu' and, per element, the spread of its 24 rounding-jittered runs (G12's model): relative noise
    of each finite element and whether its NaN mask flips."""
    from oracle import vfo_numpy as orc
    with np.errstate(all="ignore"):
        mu, mup = orc.phase_group_index(X, Y, P, mode)
        noise = [np.zeros(X.shape), np.zeros(X.shape)]
        flip = np.zeros(X.shape, dtype=bool)
        rng = np.random.default_rng(1702)
        for _ in range(runs):
            for k, (ref, jit) in enumerate(zip((mu, mup), orc.phase_group_index(X, Y, P, mode, rounding_rng=rng))):
                flip |= np.isnan(ref) != np.isnan(jit)
                ok = np.isfinite(ref) & np.isfinite(jit) & (ref != 0)
                rel = np.zeros(X.shape)
                rel[ok] = np.abs(jit[ok] - ref[ok]) / np.abs(ref[ok])
                noise[k] = np.maximum(noise[k], rel)
    return mu, mup, noise, flip


def _index_cases_g16():
    g = load_golden("g16_stage_edges.npz")
    return [(str(c), g[f"mu_{c}_X"], g[f"mu_{c}_Y"], g[f"mu_{c}_psi"]) for c in g["mu_cases"]]


def _offenders(bad, X, Y, P, got, ref):
    """(X, Y, psi, got, ref) of the first few elements a check refuses: what a failure message needs."""
    return [(float(X[i]), float(Y[i]), float(P[i]), float(got[i]), float(ref[i])) for i in np.flatnonzero(bad)[:6]]


@pytest.mark.parametrize("mode", ["O", "X"])
def test_mu_mup_faithful_tier_against_the_oracle(lib, mode):
    """~2e5 random elements and every G16 edge - infinite Y included (YT**3 and YT**4 overflow to +-inf as NumPy's pow
    does) - each case its own call (the isotropic test spans one call's array), host and unaligned device arrays.  NaN
    masks identical except where the oracle's own rounding jitter flips that element; finite elements within
    max(1e-12 for mu, 1e-10 for mu', 4 x noise) of the oracle (G12's rule, tests/parity.py).  The oracle is G16's
    reference run bit for bit (tests/test_oracle_golden.py::test_stage_ops_edges_g16)."""
    X, Y, P = _triples(200_003, 1703)
    cases = [("random", X, Y, P)] + _index_cases_g16()
    for name, X, Y, P in cases:
        mu_r, mup_r, noise, flip = _index_reference(X, Y, P, mode)
        for placement in ("host", "offset1"):
            got = _mu_mup(lib, X, Y, P, mode, TIERS["faithful"], placement)
            for k, (g, ref, tol) in enumerate(zip(got, (mu_r, mup_r), (1e-12, 1e-10))):
                where = (name, placement, ("mu", "mup")[k])
                mism = (np.isnan(g) != np.isnan(ref)) & ~flip
                assert not mism.any(), (where, int(mism.sum()), _offenders(mism, X, Y, P, g, ref))
                ok = np.isfinite(ref) & ~np.isnan(g)                 # (an infinite result fails the bound below)
                over = np.zeros(ref.shape, dtype=bool)
                over[ok] = np.abs(g[ok] - ref[ok]) > np.maximum(tol, 4.0 * noise[k][ok]) * np.abs(ref[ok])
                assert not over.any(), (where, int(over.sum()), _offenders(over, X, Y, P, g, ref))


def _index_band(X, Y, P, mode):
    """Elements whose NaN mask a last-bit difference can decide, from the reference's own intermediates
    (library.py:210-238): the radicand 1 - X (1 - X) / D within 1e-9 of 0 or 1 (the two NaN thresholds, :233, :238),
    or D within 1e-9 of the size of its terms (D changes sign there)."""
    with np.errstate(all="ignore"):
        s, c = np.sin(np.deg2rad(P)), np.cos(np.deg2rad(P))
        YT, YL, Xm1 = Y * s, Y * c, 1.0 - X
        beta = np.sqrt(0.25 * YT ** 4 + YL ** 2 * Xm1 ** 2)
        D = Xm1 - 0.5 * YT ** 2 + (1.0 if mode == "O" else -1.0) * beta
        r = 1.0 - X * Xm1 / D
        return (np.abs(r) <= 1e-9) | (np.abs(r - 1.0) <= 1e-9) | \
            (np.abs(D) <= 1e-9 * (np.abs(Xm1) + 0.5 * YT ** 2 + beta)) | ~np.isfinite(r)


def _fast_tier_limits(X, Y, P):
    """Elements at the 0 / 0 and inf / inf limits of the long form (library.py:217-254), which the reduced algebra
    (deviation (6)) takes in closed form and the reference's order does not: X exactly 0 or 1,
    psi an exact multiple of 90 degrees (YT or YL zero up to the rounding of sin / cos), Y infinite, and Y == 0 in a
    magnetised call (beta = 0).  An isotropic call - nanmax|Y| < 1e-12 - takes neither formula and bands nothing."""
    magnetised = bool(np.isnan(Y).all()) or not (np.nanmax(np.abs(Y)) < 1e-12)     # (np.nanmax of all-NaN: NaN)
    if not magnetised:
        return np.zeros(X.shape, dtype=bool)
    return (X == 0.0) | (X == 1.0) | (np.mod(P, 90.0) == 0.0) | np.isinf(Y) | (Y == 0.0)


@pytest.mark.parametrize("mode", ["O", "X"])
def test_mu_mup_fast_tier_against_the_oracle(lib, mode):
    """The fast tier on the same elements, every G16 case included: the bounds test_find_mu_mup_device_op states (1e-9
    for mu, 1e-7 for mu' where mu > 0.05, or 4 x the oracle's own noise where that is larger); NaN masks identical
    outside the bands of `_index_band` and `_fast_tier_limits` and the oracle's jitter flips."""
    X, Y, P = _triples(200_003, 1703)
    for name, X, Y, P in [("random", X, Y, P)] + _index_cases_g16():
        mu_r, mup_r, noise, flip = _index_reference(X, Y, P, mode)
        band = flip | _index_band(X, Y, P, mode) | _fast_tier_limits(X, Y, P)
        for placement in ("host", "offset1"):
            got = _mu_mup(lib, X, Y, P, mode, TIERS["fast"], placement)
            for k, (g, ref, tol) in enumerate(zip(got, (mu_r, mup_r), (1e-9, 1e-7))):
                where = (name, placement, ("mu", "mup")[k])
                mism = (np.isnan(g) != np.isnan(ref)) & ~band
                assert not mism.any(), (where, int(mism.sum()), _offenders(mism, X, Y, P, g, ref))
                well = np.isfinite(ref) & ~np.isnan(g) & (mu_r > 0.05) & ~band
                over = np.zeros(ref.shape, dtype=bool)
                over[well] = np.abs(g[well] - ref[well]) > np.maximum(tol, 4.0 * noise[k][well]) * np.abs(ref[well])
                assert not over.any(), (where, int(over.sum()), _offenders(over, X, Y, P, g, ref))


def _last_piece_start(n):
    """First element of the last workgroup's piece in mu_mup_kernel's 16-byte path (launch_mu_mup: min(ceil(n / 256),
    4096) workgroups, pairs of elements cut into equal pieces)."""
    blocks = min((n + 255) // 256, 4096)
    pairs = n >> 1
    piece = (pairs + blocks - 1) // blocks
    return 2 * (blocks - 1) * piece


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("n", [7, 2_097_153])
def test_mu_mup_isotropic_switch_spans_the_whole_array(lib, n, tier):
    """nanmax|Y| < 1e-12 over the WHOLE array (library.py:201): one |Y| >= 1e-12 anywhere - the first element, the
    last of an odd n (the odd tail), the first of the last workgroup's piece - gives the magnetised formulas
    everywhere (with Y = 0 their mu' is NaN: 0 / 0 in dbeta_dX), 0.99e-12 everywhere the isotropic ones, and an
    all-NaN Y the magnetised ones (np.nanmax -> NaN)."""
    level = TIERS[tier]
    Xp = np.random.default_rng(1704).uniform(0.0, 1.2, PERIOD)
    Pp = np.random.default_rng(1705).uniform(-90.0, 270.0, PERIOD)
    X, P = np.resize(Xp, n), np.resize(Pp, n)
    for mode in "OX":
        # magnetised with Y = 0: a small call that has one magnetised element beside the period
        mag = [v[:PERIOD] for v in lib.find_mu_mup(np.append(Xp, 0.5), np.append(np.zeros(PERIOD), 1.0),
                                                    np.append(Pp, 45.0), mode, math=level)]
        iso = lib.find_mu_mup(Xp, np.zeros(PERIOD), Pp, mode, math=level)
        assert np.isnan(mag[1]).all() and np.isfinite(iso[1]).any()          # the two answers are told apart
        for where in sorted({0, n - 1, _last_piece_start(n)}):
            for yv in (1e-12, -1e-12, 0.3):
                Y = np.zeros(n)
                Y[where] = yv
                lone = lib.find_mu_mup(np.array([X[where], 0.5]), np.array([yv, 1.0]), np.array([P[where], 45.0]),
                                       mode, math=level)
                for placement in ("host", "aligned", "offset1"):
                    got = _mu_mup(lib, X, Y, P, mode, level, placement)
                    for k in range(2):
                        want = np.resize(mag[k], n)
                        want[where] = lone[k][0]
                        assert same_bits(got[k], want), (mode, where, yv, placement, k)
        for Y, want in ((np.full(n, 0.99e-12), iso), (np.full(n, np.nan), None)):
            for placement in ("host", "aligned", "offset1"):
                got = _mu_mup(lib, X, Y, P, mode, level, placement)
                if want is None:                                               # magnetised with Y = NaN: NaN throughout
                    assert np.isnan(got[0]).all() and np.isnan(got[1]).all(), (mode, placement)
                else:
                    assert same_bits(got[0], np.resize(want[0], n)) and same_bits(got[1], np.resize(want[1], n)), \
                        (mode, placement)


VH_SHAPES = [(1, 1), (1, 2), (5, 63), (5, 64), (5, 65), (7, 129), (6, 20_001), (9, 300_000)]


def _vh_inputs(rows, cols, seed):
    """Rows of an X-mode / O-mode grid: X rising towards reflection, Y, psi and dh positive; a NaN term or two."""
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(0.0, 0.95, (rows, cols)), axis=1)
    Y = rng.uniform(0.05, 0.6, (rows, cols))
    P = rng.uniform(0.0, 180.0, (rows, cols))
    D = rng.uniform(0.1, 1.0, (rows, cols))
    if cols > 3:
        X[0, cols // 2] = 1.5                # a NaN term the sum skips (:288)
    return X, Y, P, D


def _vh_terms(X, Y, P, D, mode):
    from oracle import vfo_numpy as orc
    with np.errstate(all="ignore"):
        _, mup = orc.phase_group_index(X, Y, P, mode)
        return mup * D


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("shape", VH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_find_vh_shapes_and_placements_against_the_oracle(lib, shape, tier):
    """Row counts that are and are not a multiple of the four rows a workgroup takes, odd n_cols (the scalar path)
    and very long rows; host, aligned device and rows at an odd offset.  Against oracle.group_path: X mode within
    1e-11, O mode within max(1e-11, 4 x the row's rounding noise) (fast tier: 1e-7 / 4 x noise); across placements
    the sums may be added in another order: within 2 n_cols 2^-53 sum|terms|."""
    from oracle import vfo_numpy as orc
    rows, cols = shape
    level = TIERS[tier]
    for mode in "OX":
        X, Y, P, D = _vh_inputs(rows, cols, 1710 + cols)
        with np.errstate(all="ignore"):
            ref = orc.group_path(X, Y, P, D, 90.0, mode)
            noise = np.zeros(rows)
            rng = np.random.default_rng(1711)
            for _ in range(24 if mode == "O" else 0):
                jit = orc.group_path(X, Y, P, D, 90.0, mode, rounding_rng=rng)
                # (a row whose jittered sum turns NaN gets the cap of tests/parity.py, not an unbounded floor)
                noise = np.maximum(noise, np.where(np.isfinite(jit), np.abs(jit - ref) / np.abs(ref), LIMIT_CAP))
        tol = 1e-11 if tier == "faithful" else 1e-7
        slack = 2.0 * cols * 2.0 ** -53 * np.array([math.fsum(np.abs(t[np.isfinite(t)])) for t in _vh_terms(X, Y, P, D, mode)])
        first = None
        for placement in ("host", "aligned", "offset1"):
            got = _find_vh(lib, X, Y, P, D, 90.0, mode, level, placement)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (mode, placement)
            ok = np.isfinite(ref)
            lim = np.minimum(LIMIT_CAP, np.maximum(tol, 4.0 * noise[ok])) * np.abs(ref[ok])
            err = np.abs(got[ok] - ref[ok])
            assert (err <= lim).all(), (mode, placement, float(np.max(err / np.abs(ref[ok]))))
            if first is None:
                first = got
            else:
                assert (np.abs(got[ok] - first[ok]) <= slack[ok]).all(), (mode, placement)


def test_find_vh_g16_rows_and_whole_array_isotropic_test(lib):
    """G16's rows (all-NaN terms and dh = 0 both give NaN, only the last term finite) on every placement, and the
    isotropic test over the whole 2-D array: a lone |Y| >= 1e-12 in the LAST row switches every row."""
    g = load_golden("g16_stage_edges.npz")
    for case in g["vh_cases"]:
        a = [g[f"vh_{case}_{k}"] for k in ("X", "Y", "psi", "dh")]
        amin = float(g[f"vh_{case}_alt_min"])
        for mode in "OX":
            want = g[f"vh_{case}_vh_{mode}"]
            for placement in ("host", "aligned", "offset1"):
                got = _find_vh(lib, *a, amin, mode, TIERS["faithful"], placement)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (case, mode, placement)
                ok = np.isfinite(want)
                np.testing.assert_allclose(got[ok], want[ok], rtol=1e-11 if mode == "X" else 1e-9, err_msg=str((case, placement)))
    for rows, cols in ((5, 63), (9, 300_000)):
        X, _, P, D = _vh_inputs(rows, cols, 1720)
        X = np.minimum(X, 0.9)
        for mode in "OX":
            iso = lib.find_vh(X, np.zeros_like(X), P, D, 90.0, mode)
            assert np.isfinite(iso).all()                                    # isotropic formulas: finite mu'
            Y = np.zeros_like(X)
            Y[-1, -1] = 1e-12
            # (offset1 with odd n_cols is one call per row - see _find_vh - and cannot span the array)
            for placement in ("host", "aligned") + (("offset1",) if cols % 2 == 0 else ()):
                got = _find_vh(lib, X, Y, P, D, 90.0, mode, TIERS["faithful"], placement)
                # magnetised with Y = 0: every term NaN (0 / 0 in dbeta_dX), every row's sum zero -> NaN
                assert np.isnan(got[:-1]).all(), (rows, cols, mode, placement)
                Y[-1, -1] = 0.99e-12
                got = _find_vh(lib, X, Y, P, D, 90.0, mode, TIERS["faithful"], placement)
                np.testing.assert_allclose(got, iso, rtol=2.0 * cols * 2.0 ** -53)    # (positive terms, any order)
                Y[-1, -1] = 1e-12


# ---- regrid ----------------------------------------------------------------------------------------------------
_RG_KEYS = ("freq", "den", "bmag", "bpsi", "dist", "alt", "crit_height")


def _regrid_device(lib, fz, den, bmag, bpsi, alt, mode, n_points):
    """prhf_regrid_f64 on device pointers (outputs start as SENTINEL; `ind` as -7)."""
    import torch
    from pyrayhf_amd import _native
    ins = [_on_device(np.asarray(a, dtype=np.float64), 0) for a in (fz, den, bmag, bpsi, alt)]
    mult = _on_device(lib._multiplier(n_points), 0)
    shape = (fz.size, n_points)
    outs = [torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda") for _ in _RG_KEYS]
    ind = torch.full(shape, -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx = _native.host_context()
    _native.raise_for(ctx.regrid(ins[0].data_ptr(), fz.size, *(t.data_ptr() for t in ins[1:]), den.size,
                                 mult.data_ptr(), n_points, lib._MODE_CODE[mode],
                                 [t.data_ptr() for t in outs] + [ind.data_ptr()], _native.FLAG_DEVICE_PTRS))
    out = {k: t.cpu().numpy() for k, t in zip(_RG_KEYS, outs)}
    out["ind"] = ind.cpu().numpy()
    return out


def _check_regrid(lib, fz, den, bmag, bpsi, alt, mode, n_points, want, where):
    """Both placements bit-identical to `want` (the oracle or a reference run), ind int64 0 .. n_points - 1."""
    for placement in ("host", "device"):
        if placement == "host":
            got = lib.regrid_to_nonuniform_grid(fz, den, bmag, bpsi, alt, mode=mode, n_points=n_points)
        else:
            got = _regrid_device(lib, fz, den, bmag, bpsi, alt, mode, n_points)
        for k in _RG_KEYS:
            assert same_bits(got[k], want[k]), (where, placement, k)
        assert got["ind"].dtype == np.int64, (where, placement)
        assert np.array_equal(got["ind"], np.broadcast_to(np.arange(n_points), (fz.size, n_points))), (where, placement)


def _oracle_columns(fz, den, bmag, bpsi, alt, mode, n_points):
    from oracle import vfo_numpy as orc
    with np.errstate(all="ignore"):
        return orc.stretched_columns(fz, den, bmag, bpsi, alt, mode, n_points)


@pytest.mark.parametrize("n_points", [1, 2, 3, 511, 512, 513, 1025, 20_000])
def test_regrid_random_profiles_bit_identical_to_the_oracle(lib, n_points):
    """random_problem's profiles (ragged grids, valleys, plateaus, vacuum at the bottom, field-angle jumps), one at a
    time, with 1, 174 or 1025 frequencies, both modes, host and device pointers: bit for bit the oracle's columns."""
    from test_gpu_random import random_problem
    rng = np.random.default_rng(1730 + n_points)
    # (1025 frequencies x 20 000 points would be 1.3 GB per set of eight outputs: that grid takes 1 and 174)
    combos = [(nf, mode) for nf in ((1, 174, 1025) if n_points <= 1025 else (1, 174)) for mode in "OX"] * 2
    for trial in range(400):
        if not combos:
            break
        freq, den, bmag, bpsi, alt, _ = random_problem(rng)
        a = alt[0] if alt.ndim == 2 else alt
        if np.argmax(den[0]) == 0:
            continue                                             # (peak at level 0: the reference's IndexError)
        n_freq, mode = combos.pop()
        fz = np.sort(rng.uniform(0.2, 15.0, n_freq)) * 1e6
        want = _oracle_columns(fz, den[0], bmag[0], bpsi[0], a, mode, n_points)
        _check_regrid(lib, fz, den[0], bmag[0], bpsi[0], a, mode, n_points, want, (trial, n_freq, mode))
    assert not combos


@pytest.mark.parametrize("mode", ["O", "X"])
def test_regrid_g16_edges_bit_identical_to_the_reference(lib, mode):
    """Every G16 case (K == 1, reflection at level 0, f = 0 / NaN / escaping, X mode below f_H, valley and plateau,
    1300 ragged levels, G13's tall columns, NaN in alt / bmag / bpsi above the peak and at it, NaN-padded density),
    host and device pointers, bit for bit the reference's own arrays."""
    g = load_golden("g16_stage_edges.npz")
    for case in g["rg_cases"]:
        a = [g[f"rg_{case}_{k}_in"] for k in ("freq", "den", "bmag", "bpsi", "alt")]
        want = {k: g[f"rg_{case}_{k}_{mode}"] for k in _RG_KEYS}
        _check_regrid(lib, *a, mode, int(g[f"rg_{case}_n_points"]), want, str(case))


@pytest.mark.parametrize("case", ["tall_day", "tall_rag"])
def test_regrid_tall_columns_whole_frequency_set(lib, case):
    """G13's tall columns (3 096 and 2 600 levels; peaks at 1 290 and 667) with every frequency of the fixture and a
    NaN altitude / field value above the peak: bit for bit the oracle (pinned to the reference by G13 and G16)."""
    t = load_golden("g13_tall_nanpad.npz")
    a = {k: t[f"{case}_{k}"].copy() for k in ("den", "bmag", "bpsi", "alt")}
    fz = t[f"{case}_freq"] * 1e6
    peak = int(np.argmax(a["den"]))
    for mode, n in (("O", 200), ("X", 513)):
        want = _oracle_columns(fz, a["den"], a["bmag"], a["bpsi"], a["alt"], mode, n)
        _check_regrid(lib, fz, a["den"], a["bmag"], a["bpsi"], a["alt"], mode, n, want, (case, mode))
        b = {k: v.copy() for k, v in a.items()}
        b["alt"][[peak, peak + 700]] = np.nan
        b["bmag"][peak + 1] = np.nan
        b["bpsi"][-1] = np.nan
        _check_regrid(lib, fz, b["den"], b["bmag"], b["bpsi"], b["alt"], mode, n, want, (case, mode, "nan above"))


def test_regrid_refusals(lib):
    """A NaN in alt, bmag or bpsi BELOW the peak is still refused (prhf.h), and a bottomside taller than the 1400
    levels LDS holds (G13 tall_fine: peak at level 2 580) raises a ValueError that names that limit, host and device."""
    import torch
    d = load_golden("g4_day_night.npz")
    fz = np.array([2.0e6, 5.0e6])
    for col, level in (("alt", 100), ("bmag", 10), ("bpsi", 257)):
        a = {k: d[f"Day_{k}"].copy() for k in ("den", "bmag", "bpsi", "alt")}
        a[col][level] = np.nan
        for mode in "OX":
            with pytest.raises(ValueError, match="NaN"):
                lib.regrid_to_nonuniform_grid(fz, a["den"], a["bmag"], a["bpsi"], a["alt"], mode=mode, n_points=20)
    t = load_golden("g13_tall_nanpad.npz")
    a = [t[f"tall_fine_{k}"] for k in ("den", "bmag", "bpsi", "alt")]
    with pytest.raises(ValueError, match="1400-level bottomside limit"):
        lib.regrid_to_nonuniform_grid(fz, *a, mode="O", n_points=20)
    with pytest.raises(ValueError, match="1400-level bottomside limit"):
        _regrid_device(lib, fz, *a, "X", 20)
    torch.cuda.synchronize()
    # one level below the limit regrids (peak at level 1399 of a 2000-level column), host and device
    alt = 80.0 + 0.1 * np.arange(2000)
    den = 1e12 * np.exp(-0.5 * ((alt - alt[1399]) / 30.0) ** 2)
    den[1399] *= 1.0001
    bm, bp = np.full(2000, 4e-5), np.full(2000, 60.0)
    want = _oracle_columns(fz, den, bm, bp, alt, "O", 33)
    _check_regrid(lib, fz, den, bm, bp, alt, "O", 33, want, "peak at 1399")
    den[1400] = 2e12
    with pytest.raises(ValueError, match="1400-level bottomside limit"):
        lib.regrid_to_nonuniform_grid(fz, den, bm, bp, alt, mode="O", n_points=20)
