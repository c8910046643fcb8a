"""Many ionograms in one launch (DESIGN.md 4.5 "many ionograms"): the masked residual stage against the existing
single-trace kernel bit for bit, the per-ionogram argmin, the fused call against the loop of today's calls, the
reference's own residual rows (fixture G11), minimize_parameters_many against minimize_parameters, and the guard of
a device-resident ionogram_of_row."""

import numpy as np
import pytest

from conftest import load_golden, same_bits

pytestmark = pytest.mark.gpu

F_SIZES = (1, 63, 64, 65, 130)
GROUP_SIZES = (0, 1, 3, 5)


# ---- 1. the stage against residual_kernel, bit for bit -----------------------------------------------------------------
def _masks(F):
    """Kept sets with 0, 1, 63, 64, 65 and F members (those that fit): "all kept", "only the last kept", and for the
    other counts a random choice."""
    rng = np.random.default_rng(100 + F)
    masks = []
    for count in sorted({c for c in (0, 1, 63, 64, 65, F) if c <= F}):
        m = np.zeros(F, dtype=bool)
        if count == 1:
            m[-1] = True                                   # only the last kept
        elif count == F:
            m[:] = True                                    # all kept
        else:
            m[rng.choice(F, size=count, replace=False)] = True
        masks.append(m)
    return masks


def _stage_case(F):
    """Ionograms (each mask twice, so that every mask meets a group that is not empty), ragged groups of 0, 1, 3 and 5
    rows, model traces with NaNs at chosen places."""
    rng = np.random.default_rng(F)
    once = _masks(F)
    masks = once * 2
    n_iono = len(masks)
    sizes = [GROUP_SIZES[k % 4] for k in range(len(once))] + [GROUP_SIZES[(k + 1) % 4] for k in range(len(once))]
    ion = np.repeat(np.arange(n_iono, dtype=np.int32), sizes)
    P = ion.size
    assert P % 4 != 0 and all(any(sizes[i] for i in range(n_iono) if masks[i] is m) for m in masks)
    obs = rng.uniform(150.0, 450.0, (n_iono, F))
    for i, m in enumerate(masks):
        obs[i, ~m] = np.nan
    obs[1 % n_iono, 0] = np.inf if not masks[1 % n_iono][0] else obs[1 % n_iono, 0]     # not finite: not kept either
    model = rng.uniform(90.0, 600.0, (P, F))
    model[rng.random((P, F)) < 0.2] = np.nan               # escapes, at kept and at masked frequencies alike
    model[0] = np.nan                                      # a candidate none of whose frequencies reflects
    model[P - 1, : F // 2] = np.nan
    model[P // 2] = rng.uniform(1.0, 60.0, F)              # mean |vh| < 100: the floor of the fill ...
    model[P // 2, ::2] = np.nan                            # ... is what fills
    return masks, ion, obs, model


_reference = {}


def _existing_entry(F):
    """What prhf_residual_f64 - the existing entry - gives on the compacted rows: per ionogram with a kept frequency,
    (residual (P, |K_i|), cost (P,)) of ALL model rows against its compacted trace.  Computed once per F."""
    if F not in _reference:
        from pyrayhf_amd import _native
        masks, ion, obs, model = _stage_case(F)
        ctx = _native.host_context(0)
        ref = {}
        for i, m in enumerate(masks):
            if not m.any():
                continue
            keep = np.isfinite(obs[i])
            assert np.array_equal(keep, m)
            vm, vo = np.ascontiguousarray(model[:, keep]), np.ascontiguousarray(obs[i, keep])
            res, cost = np.empty_like(vm), np.empty(model.shape[0])
            _native.raise_for(ctx.residual(vm.ctypes.data, vo.ctypes.data, vm.shape[0], vm.shape[1], res.ctypes.data,
                                           cost.ctypes.data, 0))
            ref[i] = (res, cost)
        _reference[F] = (masks, ion, obs, model, ref)
    return _reference[F]


def _first_finite_min(cost):
    finite = np.isfinite(cost)
    if not finite.any():
        return -1, np.nan
    k = int(np.argmin(np.where(finite, cost, np.inf)))
    return k, cost[k]


def _run_stage(model, obs, ion, device_ptrs, want_residual=True):
    """prhf_residual_many_f64 on host arrays or on device tensors; results as NumPy arrays."""
    from pyrayhf_amd import _native
    P, F = model.shape
    n_iono = obs.shape[0]
    shared = ion is None
    if not device_ptrs:
        model, obs = np.ascontiguousarray(model), np.ascontiguousarray(obs)
        cost = np.full((n_iono, P) if shared else P, -7.0)
        best, best_cost = np.full(n_iono, -7, dtype=np.int64), np.full(n_iono, -7.0)
        res = np.full((P, F), -7.0) if want_residual and not shared else None
        _native.raise_for(_native.host_context(0).residual_many(
            model.ctypes.data, P, obs.ctypes.data, n_iono, F, None if shared else ion.ctypes.data,
            None if res is None else res.ctypes.data, cost.ctypes.data, best.ctypes.data, best_cost.ctypes.data, 0))
        return res, cost, best, best_cost
    import torch
    dev = torch.device("cuda:0")
    t_model, t_obs = torch.as_tensor(model, device=dev).contiguous(), torch.as_tensor(obs, device=dev).contiguous()
    t_ion = None if shared else torch.as_tensor(ion, device=dev)
    cost = torch.full((n_iono, P) if shared else (P,), -7.0, dtype=torch.float64, device=dev)
    best = torch.full((n_iono,), -7, dtype=torch.int64, device=dev)
    best_cost = torch.full((n_iono,), -7.0, dtype=torch.float64, device=dev)
    res = torch.full((P, F), -7.0, dtype=torch.float64, device=dev) if want_residual and not shared else None
    ctx = _native.context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _native.raise_for(ctx.residual_many(t_model.data_ptr(), P, t_obs.data_ptr(), n_iono, F,
                                        None if shared else t_ion.data_ptr(), None if res is None else res.data_ptr(),
                                        cost.data_ptr(), best.data_ptr(), best_cost.data_ptr(), _native.FLAG_DEVICE_PTRS))
    torch.cuda.synchronize()
    return (None if res is None else res.cpu().numpy(), cost.cpu().numpy(), best.cpu().numpy(), best_cost.cpu().numpy())


@pytest.mark.parametrize("device_ptrs", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("F", F_SIZES)
def test_stage_own_candidates_equal_the_existing_kernel_bit_for_bit(F, device_ptrs):
    masks, ion, obs, model, ref = _existing_entry(F)
    res, cost, best, best_cost = _run_stage(model, obs, ion, device_ptrs)
    for p in range(model.shape[0]):
        i = int(ion[p])
        keep = masks[i]
        assert np.isnan(res[p, ~keep]).all()                              # not kept: NaN
        if not keep.any():
            assert np.isnan(cost[p])                                      # an empty K_i: NaN cost
            continue
        want_res, want_cost = ref[i]
        assert same_bits(res[p, keep], want_res[p]), (F, p)
        assert same_bits(cost[p], want_cost[p]), (F, p, cost[p], want_cost[p])
    for i in range(len(masks)):
        rows = np.nonzero(ion == i)[0]
        k, c = _first_finite_min(cost[rows])
        assert best[i] == (rows[k] if k >= 0 else -1) and same_bits(best_cost[i], c), (F, i)      # a GLOBAL row
    # without the dense residual output: the same costs
    _, cost2, best2, best_cost2 = _run_stage(model, obs, ion, device_ptrs, want_residual=False)
    assert same_bits(cost2, cost) and np.array_equal(best2, best) and same_bits(best_cost2, best_cost)


@pytest.mark.parametrize("device_ptrs", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("F", F_SIZES)
def test_stage_shared_candidates_equal_the_existing_kernel_bit_for_bit(F, device_ptrs):
    masks, _, obs, model, ref = _existing_entry(F)
    _, cost, best, best_cost = _run_stage(model, obs, None, device_ptrs)
    assert cost.shape == (len(masks), model.shape[0])
    for i, keep in enumerate(masks):
        if not keep.any():
            assert np.isnan(cost[i]).all() and best[i] == -1 and np.isnan(best_cost[i])
            continue
        assert same_bits(cost[i], ref[i][1]), (F, i)
        k, c = _first_finite_min(ref[i][1])
        assert best[i] == k and same_bits(best_cost[i], c)


# ---- 2. argmin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_ptrs", [False, True], ids=["host", "device"])
def test_best_is_the_first_row_of_the_smallest_finite_cost(device_ptrs):
    rng = np.random.default_rng(2)
    F = 70
    # groups: 0 - 70 rows with duplicates (more than one trip of the wave over the rows), 1 - every cost NaN,
    # 2 - empty, 3 - one row, 4 - duplicates of the winner at its end, 5 - no observation at all, 6 - the last rows
    sizes = [70, 3, 0, 1, 6, 2, 4]
    ion = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    P = ion.size
    obs = rng.uniform(200.0, 300.0, (len(sizes), F))
    obs[:, ::5] = np.nan
    obs[5] = np.nan
    model = rng.uniform(150.0, 350.0, (P, F))
    first = np.concatenate([[0], np.cumsum(sizes)])
    near = np.where(np.isnan(obs[0]), 0.0, obs[0]) + 0.5
    model[first[0] + 66] = near                            # the winner of group 0, in the wave's second trip ...
    model[first[0] + 69] = near                            # ... and its duplicates behind it and ...
    model[first[0] + 67] = near
    model[first[1]:first[2]] = np.nan                      # group 1: nothing reflects: NaN fill, NaN costs
    model[first[4] + 2] = np.where(np.isnan(obs[4]), 0.0, obs[4]) - 0.25
    model[first[4] + 5] = model[first[4] + 2]
    model[first[4] + 3] = model[first[4] + 2]
    res, cost, best, best_cost = _run_stage(model, obs, ion, device_ptrs)
    assert cost[first[0] + 66] == cost[first[0] + 67] == cost[first[0] + 69] == np.nanmin(cost[first[0]:first[1]])
    assert best[0] == first[0] + 66                        # a tie goes to the lowest row
    assert np.isnan(cost[first[1]:first[2]]).all() and best[1] == -1 and np.isnan(best_cost[1])
    assert best[2] == -1 and np.isnan(best_cost[2])        # an empty group
    assert best[3] == first[3] and best_cost[3] == cost[first[3]] and np.isfinite(cost[first[3]])   # a group of one
    assert best[4] == first[4] + 2 and cost[first[4] + 2] == cost[first[4] + 3] == cost[first[4] + 5]
    assert best[5] == -1 and np.isnan(best_cost[5]) and np.isnan(cost[first[5]:first[6]]).all()
    k, c = _first_finite_min(cost[first[6]:])
    assert best[6] == first[6] + k and best_cost[6] == c and best[6] >= P - 4       # global row indices
    for i in (0, 4):
        assert best_cost[i] == cost[best[i]]
    # shared candidates: the same rows against every ionogram; the winner is the candidate index
    _, cost_s, best_s, best_cost_s = _run_stage(model, obs, None, device_ptrs)
    for i in range(len(sizes)):
        k, c = _first_finite_min(cost_s[i])
        assert best_s[i] == k and same_bits(best_cost_s[i], c)
    assert best_s[0] == first[0] + 66 and best_s[4] == first[4] + 2 and best_s[5] == -1


# ---- 3. end to end against the loop of today's calls -------------------------------------------------------------------------
def _site(n_alt=60):
    alt = np.linspace(80.0, 375.0, n_alt)
    bmag = 4.6e-5 * ((6371.0 + 80.0) / (6371.0 + alt)) ** 3
    bpsi = 35.0 + 0.01 * (alt - alt[0])
    return alt, bmag, bpsi


def _layer(alt, nm, hm, h):
    z = (alt - hm) / h
    ze = (alt - 110.0) / 8.0
    return nm * np.exp(0.5 * (1.0 - z - np.exp(-z))) + 4e10 * np.exp(0.5 * (1.0 - ze - np.exp(-ze)))


def _end_to_end_case(F, mode, n_points):
    from pyrayhf_amd import library
    alt, bmag, bpsi = _site()
    freq = np.array([4.0]) if F == 1 else np.linspace(1.5, 9.5, F)
    sizes = [5, 3, 1, 4]                                   # ragged groups; 13 rows
    ion = np.repeat(np.arange(4, dtype=np.int32), sizes)
    hms = [250.0, 262.0, 274.0, 286.0, 298.0, 255.0, 270.0, 285.0, 280.0, 260.0, 272.0, 284.0, 296.0]
    nms = [9e11, 8e11, 7e11, 9.5e11, 6e11, 8e11, 9e11, 7e11, 8.5e11, 9e11, 8e11, 7.5e11, 6.5e11]
    den = np.array([_layer(alt, nm, hm, 38.0) for nm, hm in zip(nms, hms)])
    winners = [2, 6, 8, 12]                                # one candidate of each group
    traces = library.vertical_forward_operator(freq, den[winners], bmag, bpsi, alt, mode, n_points)
    obs = np.where(np.isnan(traces), 420.0, traces) + np.array([0.25, -0.5, 0.125, 0.75])[:, None]
    obs[0, 1::4] = np.nan                                  # every ionogram has a mask of its own
    obs[1, ::3] = np.nan
    obs[3, F // 2:F // 2 + 7] = np.nan
    if F == 1:
        obs[:] = (np.where(np.isnan(traces), 420.0, traces) + 0.25)
    return freq, obs, den, ion, alt, bmag, bpsi, winners


@pytest.mark.parametrize("mode,n_points", [("O", 2), ("O", 200), ("X", 2), ("X", 200)])
@pytest.mark.parametrize("F", F_SIZES)
def test_fused_call_equals_the_loop_of_single_trace_calls(F, mode, n_points):
    from pyrayhf_amd import fitting
    freq, obs, den, ion, alt, bmag, bpsi, _ = _end_to_end_case(F, mode, n_points)
    cost, best, best_cost, res, vh = fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, mode, n_points,
                                                              ionogram_of_row=ion, return_residual=True, return_vh=True)
    assert cost.shape == (13,) and best.shape == best_cost.shape == (4,) and res.shape == vh.shape == (13, F)
    bit_equal = True
    for i in range(4):
        rows = np.nonzero(ion == i)[0]
        keep = np.isfinite(obs[i])
        assert keep.any()
        want_res, want_cost = fitting.residual_VH_batch(freq[keep], obs[i, keep], den[rows], bmag, bpsi, alt, mode, n_points)
        got = res[rows][:, keep]
        assert np.isnan(res[rows][:, ~keep]).all()
        assert np.array_equal(np.isnan(got), np.isnan(want_res))
        ok = np.isfinite(want_res)
        height = np.abs(obs[i, keep][None, :] - want_res)                  # |vh|: the modeled height, or its fill
        err = np.abs(got - want_res)[ok]
        cost_ok = np.isfinite(want_cost)
        assert np.array_equal(np.isnan(cost[rows]), ~cost_ok)
        cost_err = np.abs(cost[rows] - want_cost)[cost_ok] / np.abs(want_cost[cost_ok])
        print(f"F={F} {mode}/{n_points} ionogram {i}: max |dres| {err.max() if err.size else 0.0:.3e}, "
              f"max rel dcost {cost_err.max() if cost_err.size else 0.0:.3e}")
        assert np.all(err <= 1e-10 * height[ok])
        assert np.all(cost_err <= 1e-10)
        bit_equal = bit_equal and same_bits(got, want_res) and same_bits(cost[rows], want_cost)
        # a clear winner, or the comparison of the argmin would rest on rounding
        finite = np.sort(want_cost[cost_ok])
        assert finite.size >= 1
        if finite.size > 1:
            assert finite[1] - finite[0] > 1e-6, (F, mode, n_points, i, finite[:2])
        k, c = _first_finite_min(want_cost)
        assert best[i] == rows[k] and abs(best_cost[i] - c) <= 1e-10 * abs(c)
    print(f"F={F} {mode}/{n_points}: bit equal to the loop: {bit_equal}")
    # an unsorted grid is sorted once, the observations with it: the same answer, columns ascending
    order = np.random.default_rng(F).permutation(F)
    cost_u, best_u, best_cost_u, res_u = fitting.residual_VH_many(freq[order], obs[:, order], den, bmag, bpsi, alt, mode,
                                                                  n_points, ionogram_of_row=ion, return_residual=True)
    assert same_bits(cost_u, cost) and np.array_equal(best_u, best) and same_bits(res_u, res)
    # brute_force_fit_many: the winners' traces as the operator returns them (NaN where a frequency escapes)
    b, bc, vh_best, f_sorted = fitting.brute_force_fit_many(freq[order], obs[:, order], den, bmag, bpsi, alt, mode, n_points,
                                                            ionogram_of_row=ion)
    assert np.array_equal(b, best) and same_bits(bc, best_cost) and np.array_equal(f_sorted, freq)
    assert same_bits(vh_best, vh[best])


def test_shared_candidates_and_per_ionogram_fields_equal_the_loop():
    """The shared layout (one operator run on C x F) against the loop over ionograms, and own candidates with one field
    row per ionogram against the same rows expanded by hand."""
    from pyrayhf_amd import fitting
    freq, obs, den, ion, alt, bmag, bpsi, _ = _end_to_end_case(65, "X", 200)
    cost, best, best_cost = fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, "X", 200, shared=True)
    assert cost.shape == (4, 13)
    for i in range(4):
        keep = np.isfinite(obs[i])
        _, want = fitting.residual_VH_batch(freq[keep], obs[i, keep], den, bmag, bpsi, alt, "X", 200)
        ok = np.isfinite(want)
        assert np.array_equal(np.isnan(cost[i]), ~ok) and np.all(np.abs(cost[i] - want)[ok] <= 1e-10 * np.abs(want[ok]))
        k, c = _first_finite_min(want)
        assert best[i] == k and abs(best_cost[i] - c) <= 1e-10 * abs(c)
    fields_b = np.array([bmag * (1.0 + 0.01 * i) for i in range(4)])
    fields_p = np.array([bpsi + i for i in range(4)])
    a = fitting.residual_VH_many(freq, obs, den, fields_b, fields_p, alt, "X", 200, ionogram_of_row=ion, return_residual=True)
    b = fitting.residual_VH_many(freq, obs, den, fields_b[ion], fields_p[ion], alt, "X", 200, ionogram_of_row=ion,
                                 return_residual=True)
    for x, y in zip(a, b):
        assert same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)
    assert not same_bits(a[0], fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, "X", 200, ionogram_of_row=ion)[0])


# ---- 4. the reference's own residual rows (fixture G11) ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["O", "X"])
def test_reference_rows_g11_whole_and_masked(mode):
    from pyrayhf_amd import fitting
    g = load_golden("g11_residual.npz")
    name = "grid"
    freq, obs0, want = g[f"{name}_freq"], g[f"{name}_{mode}_vh_obs"], g[f"{name}_{mode}_residual"]
    # (X mode: the fixture's trace has no echo at its two lowest frequencies - the reference's rows are NaN there, and
    #  "everything kept" keeps what there is; no candidate reflects there either, so the fill is the reference's)
    assert np.all(np.diff(freq) > 0) and np.isfinite(obs0).sum() >= 30
    edp = g[f"{name}_edp"]
    n = edp.shape[0]
    obs = np.stack([obs0, obs0])
    obs[1, ::3] = np.nan                                   # ionogram 1: every third observation missing
    den = np.concatenate([edp, edp])
    ion = np.repeat(np.arange(2, dtype=np.int32), n)
    cost, best, best_cost, res, vh = fitting.residual_VH_many(freq, obs, den, g[f"{name}_bmag"], g[f"{name}_bpsi"],
                                                              g[f"{name}_alt"], mode, int(g[f"{name}_{mode}_n_points"]),
                                                              ionogram_of_row=ion, return_residual=True, return_vh=True)
    keep1 = np.isfinite(obs[1])
    # ionogram 1: the rows whose fill never enters a kept residual - every row whose modeled trace has no NaN, and (X
    # mode, where no trace has an echo below the gyro cut-off and the fixture's observations have none there either)
    # every row whose NaNs all lie at frequencies that are not kept
    no_nan = ~np.isnan(vh[n:][:, keep1]).any(axis=1)
    assert no_nan.any() and np.isnan(res[n:][:, ~keep1]).all()
    whole = (res[:n], want, np.ones_like(want, dtype=bool), True)
    masked = (res[n:], want, no_nan[:, None] & keep1[None, :], False)
    for got, ref, where, is_whole in (whole, masked):
        assert np.array_equal(np.isnan(got)[where], np.isnan(ref)[where])
        ok = np.isfinite(ref) & where
        # the bounds of tests/test_gpu_fitting.py::test_residual_rows_match_the_reference_g11
        if mode == "X":
            scale = np.abs(np.broadcast_to(obs0, ref.shape)[ok]) + np.abs(ref[ok])
            err = np.abs(got[ok] - ref[ok]) / scale
            assert err.max() <= 1e-8, err.max()
        else:
            from parity import assert_o_mode, combined_noise
            floor = combined_noise(g[f"{name}_O_noise"], g[f"{name}_O_noise_rounding"])
            height = np.abs(g[f"{name}_O_vh_model"])
            limit = np.minimum(1e-3, np.maximum(1e-6, 4.0 * floor))
            both = ok & np.isfinite(g[f"{name}_O_vh_model"])
            assert both.any() and np.all(np.abs(got[both] - ref[both]) <= limit[both] * height[both])
            if is_whole:
                assert_o_mode(vh[:n], g[f"{name}_O_vh_model"], floor)
    finite = np.isfinite(cost[:n])
    np.testing.assert_allclose(cost[:n][finite], np.nansum(want ** 2, axis=1)[finite], rtol=1e-3 if mode == "O" else 1e-7,
                               atol=1e-6)
    assert best[0] == _first_finite_min(cost[:n])[0] and best[1] == n + _first_finite_min(cost[n:])[0]


# ---- 5. minimize_parameters_many --------------------------------------------------------------------------------------------------
def _chapman_builder(F2, F1, E, alt, bottom_type):
    """The stand-in for the reference's PyIRI EDP builders that tests/test_gpu_fitting.py uses."""
    thick = F2['B_bot'] if bottom_type == 'B_bot' else F2['B0']
    z = (alt - F2['hm'].ravel()[0]) / thick.ravel()[0]
    ze = (alt - E['hm'].ravel()[0]) / E['B_bot'].ravel()[0]
    return (F2['Nm'].ravel()[0] * np.exp(0.5 * (1.0 - z - np.exp(-z)))
            + E['Nm'].ravel()[0] * np.exp(0.5 * (1.0 - ze - np.exp(-ze))))


def _layer_dicts(nm, hm, bb):
    one = lambda v: np.array([[[v]]])                                           # noqa: E731
    return ({"Nm": one(nm), "hm": one(hm), "B_bot": one(bb)}, {"Nm": one(0.0), "hm": one(200.0), "B_bot": one(30.0)},
            {"Nm": one(3e10), "hm": one(110.0), "B_bot": one(8.0)})


@pytest.mark.parametrize("mode", ["O", "X"])
def test_minimize_parameters_many_equals_minimize_parameters(mode):
    from pyrayhf_amd import fitting, library
    alt = np.arange(80.0, 500.0, 1.0)
    b_mag = 4.6e-5 * ((6371.0 + 80.0) / (6371.0 + alt)) ** 3
    b_psi = 35.0 + 0.002 * (alt - alt[0])
    freq = np.arange(1.5, 9.0, 0.25)[::-1].copy()          # a common grid that is not sorted
    starts = [(312.0, 40.0), (300.0, 44.0), (322.0, 36.0)]                  # different initial hmF2 (and B_bot)
    F2s, F1s, Es, obs = [], [], [], []
    for i, (hm0, bb0) in enumerate(starts):
        hm_nodes, bb_nodes = fitting.brute_grid(hm0, 4.0, 2.0), fitting.brute_grid(bb0, 4.0, 2.0)
        nm = fitting.peak_density_from_trace(freq.max(), mode, alt=alt, bmag=b_mag, hmf2=hm0)
        truth = _chapman_builder(_layer_dicts(nm, hm_nodes[3 + i], bb_nodes[-1])[0], *_layer_dicts(nm, hm0, bb0)[1:], alt, 'B_bot')
        trace = library.vertical_forward_operator(freq, truth, b_mag, b_psi, alt, mode, 200)
        F2, F1, E = _layer_dicts(1.0e12, hm0, bb0)
        F2s.append(F2), F1s.append(F1), Es.append(E), obs.append(trace)
    obs = np.array(obs)
    obs[0, 4] = np.nan                                     # different masks
    obs[1, 1::5] = np.nan
    obs[2, :3] = np.nan                                    # the three highest frequencies: NmF2 from the fourth
    assert (np.isfinite(obs).sum(axis=1) >= 15).all()
    got = fitting.minimize_parameters_many(F2s, F1s, Es, freq, obs, alt, b_mag, b_psi, 4.0, 2.0, mode, 200, 'B_bot',
                                           edp_builder=_chapman_builder)
    assert len(got) == 3
    for i in range(3):
        vh, edp, F2_fit = fitting.minimize_parameters(F2s[i], F1s[i], Es[i], freq, obs[i], alt, b_mag, b_psi, 'brute', 4.0,
                                                      2.0, mode, 200, 'B_bot', edp_builder=_chapman_builder)
        vh_m, edp_m, F2_m = got[i]
        for key in ("Nm", "hm", "B_bot"):
            assert F2_m[key].shape == F2_fit[key].shape and np.array_equal(F2_m[key], F2_fit[key]), (i, key)
        assert np.array_equal(edp_m, edp) and vh_m.shape == freq.shape
        assert np.array_equal(np.isnan(vh_m), np.isnan(vh))
        ok = np.isfinite(vh)
        assert ok.sum() >= 15 and np.all(np.abs(vh_m - vh)[ok] <= 1e-10 * np.abs(vh[ok]))
        assert float(F2s[i]['hm'].squeeze()) == starts[i][0]                # the inputs are not mutated
    print(mode, "fitted (hmF2, B_bot):", [(float(f['hm'].squeeze()), float(f['B_bot'].squeeze())) for _, _, f in got])


def test_torch_resident_call_returns_device_tensors_and_agrees():
    import torch
    from pyrayhf_amd import fitting
    freq, obs, den, ion, alt, bmag, bpsi, _ = _end_to_end_case(65, "O", 200)
    want = fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, "O", 200, ionogram_of_row=ion, return_residual=True,
                                    return_vh=True)
    dev = torch.device("cuda:0")
    got = fitting.residual_VH_many(freq, torch.as_tensor(obs, device=dev), torch.as_tensor(den, device=dev),
                                   torch.as_tensor(bmag, device=dev), bpsi, alt, "O", 200,
                                   ionogram_of_row=torch.as_tensor(ion, device=dev), return_residual=True, return_vh=True)
    assert got[1].dtype == torch.int64
    for a, b in zip(got, want):
        assert a.is_cuda and a.shape == b.shape
        a = a.cpu().numpy()
        assert same_bits(a, b) if b.dtype == np.float64 else np.array_equal(a, b)
    shared_want = fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, "O", 200, shared=True)
    shared_got = fitting.residual_VH_many(freq, obs, torch.as_tensor(den, device=dev), bmag, bpsi, alt, "O", 200, shared=True)
    for a, b in zip(shared_got, shared_want):
        assert a.is_cuda and (same_bits(a.cpu().numpy(), b) if b.dtype == np.float64 else np.array_equal(a.cpu().numpy(), b))
    fit = fitting.brute_force_fit_many(freq, obs, torch.as_tensor(den, device=dev), bmag, bpsi, alt, "O", 200,
                                       ionogram_of_row=ion)
    assert fit[2].is_cuda and same_bits(fit[2].cpu().numpy(), want[4][want[1]])


# ---- 6. a device-resident ionogram_of_row is never trusted -------------------------------------------------------------------------
def test_out_of_range_device_index_gives_a_nan_cost_and_reads_nothing_outside_vh_obs():
    """The entry that names no ionogram would, unclamped, read (index x F) doubles past the observations: the
    observations are a slice in the middle of a larger NaN-filled tensor, so that even then every address is allocated
    memory.  Its row gets a NaN cost and NaN residuals; every other row and every winner is what the clean call gives.
    (The bad entries sit at the ends, where they leave the array non-decreasing: an array out of order breaks another
    part of the contract, and the winner's search may then miss rows.)"""
    import torch
    from pyrayhf_amd import _native
    rng = np.random.default_rng(6)
    F, n_iono = 65, 3
    ion = np.array([0, 0, 1, 1, 1, 2, 2], dtype=np.int32)
    obs = rng.uniform(200.0, 300.0, (n_iono, F))
    obs[:, ::4] = np.nan
    model = rng.uniform(150.0, 350.0, (ion.size, F))
    clean = _run_stage(model, obs, ion, True)
    dev = torch.device("cuda:0")
    for bad_row, bad_value in ((6, 5), (0, -2), (6, n_iono)):
        bad = ion.copy()
        bad[bad_row] = bad_value
        big = torch.full((16, F), float("nan"), dtype=torch.float64, device=dev)
        big[6:6 + n_iono] = torch.as_tensor(obs, device=dev)
        t_obs = big[6:6 + n_iono]                          # rows -6 .. 9 around it are allocated
        assert t_obs.is_contiguous() and -6 <= bad_value < 10
        t_model, t_ion = torch.as_tensor(model, device=dev), torch.as_tensor(bad, device=dev)
        cost = torch.zeros(ion.size, dtype=torch.float64, device=dev)
        res = torch.zeros((ion.size, F), dtype=torch.float64, device=dev)
        best = torch.zeros(n_iono, dtype=torch.int64, device=dev)
        best_cost = torch.zeros(n_iono, dtype=torch.float64, device=dev)
        ctx = _native.context(0)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        _native.raise_for(ctx.residual_many(t_model.data_ptr(), ion.size, t_obs.data_ptr(), n_iono, F, t_ion.data_ptr(),
                                            res.data_ptr(), cost.data_ptr(), best.data_ptr(), best_cost.data_ptr(),
                                            _native.FLAG_DEVICE_PTRS))
        torch.cuda.synchronize()
        cost, res, best, best_cost = cost.cpu().numpy(), res.cpu().numpy(), best.cpu().numpy(), best_cost.cpu().numpy()
        others = np.arange(ion.size) != bad_row
        assert np.isnan(cost[bad_row]) and np.isnan(res[bad_row]).all()
        assert same_bits(cost[others], clean[1][others]) and same_bits(res[others], clean[0][others])
        for i in range(n_iono):
            rows = np.nonzero((ion == i) & others)[0]
            k, c = _first_finite_min(cost[rows])
            assert best[i] == rows[k] and best_cost[i] == c
