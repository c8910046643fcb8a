"""What the C entry points of the operator, of its residual stages and of the un-fused stage ops refuse, which rejection
wins where two apply, and that a refused call leaves the context usable - the other half of
test_gpu_tracer_abi_rejections.py, whose ``_run``, ``_ptr``, ``ctx`` and ``null_ctx`` this module reuses.  library.py
validates before it calls, so these rejections are reached through the raw ``Context`` only.

Per entry point: the smallest valid host-buffer call - 2 profiles x 3 frequencies x a 16-point grid of g1_basic.npz, 2
ionograms, a 4 x 4 field at two frequencies - then a table of cases.  A case changes the named arguments of the valid call
and states ``(rc, part of prhf_last_error)``; every case returns before the library reads an array it was not given and
before any launch.  A case with two faults pins the order of the checks.  After its table the entry point makes the valid
call once more: OK and a finite first output."""

import numpy as np
import pytest

from test_gpu_tracer_abi_rejections import (BAD_FLAG, BIG, _deriv_base, _down_mult, _head, _native, _ptr, _run, ctx,  # noqa: F401
                                            null_ctx)

pytestmark = pytest.mark.gpu

F64 = lambda *v: np.array(v, dtype=np.float64)        # noqa: E731
I32 = lambda *v: np.array(v, dtype=np.int32)          # noqa: E731
I64 = lambda *v: np.array(v, dtype=np.int64)          # noqa: E731
ASYNC, GRID_STABLE, SHARED_FIELD = 0x2, 0x4, 0x8      # PRHF_FLAG_* of include/prhf.h (_native.FLAG_*)
MANY_MAX_FREQ = 4096                                  # PRHF_MANY_MAX_FREQ


def _base():
    import torch
    n = _native()
    a = _deriv_base()
    n_alt = a["n_alt"]
    seg = n.Segment(0, 2, n.MODE_O, 16, 0, 0)
    axis = F64(0.0, 1.0, 2.0, 3.0)
    a.update(
        segs=[seg], n_segs=1, mult_len=16,
        vh_obs=F64(100.0, 110.0, 120.0), residual=np.zeros((2, 3)), cost=np.zeros(2),
        n_iono=2, many_obs=np.array([[100.0, 110.0, 120.0], [105.0, 115.0, 125.0]]), ion=I32(0, 1),
        many_cost=np.zeros(2), best=np.zeros(2, dtype=np.int64), best_cost=np.zeros(2),
        vh_model=np.array([[101.0, 111.0, 121.0], [104.0, 114.0, 124.0]]),
        # mu_mup on 4 points, find_vh on 2 rows of 4
        X=np.tile(F64(0.1, 0.3, 0.5, 0.7), (2, 1)), Y=np.full((2, 4), 0.3), psi=np.full((2, 4), 60.0), dh=np.full((2, 4), 1.0),
        n=4, n_rows=2, n_cols=4, alt_min=100.0, mu=np.zeros(4), mup=np.zeros(4), find_out=np.zeros(2),
        # regrid of the first profile
        freq_hz=a["freq"] * 1e6, den1=a["den"][0].copy(), bmag1=a["bmag"][0].copy(), bpsi1=a["bpsi"][0].copy(),
        regrid_out=[np.zeros((3, 16)) for _ in range(7)] + [np.zeros((3, 16), dtype=np.int64)],
        # a 4 x 4 field at two frequencies
        n_fields=2, n0=4, n1=4, axis0=axis, axis1=axis.copy(), edge_order=2,
        field_mu=np.full((2, 4, 4), 0.9), field_mup=np.full((2, 4, 4), 1.1),
        records=torch.ones((2, 4, 4, 4), dtype=torch.float64, device="cuda:0"), rec_host=np.zeros((2, 4, 4, 4)),
        p0=F64(0.5, 1.5, 2.5), p1=F64(2.5, 1.5, 0.5), field_index=I64(0, 1, 0), n_samples=3, fills=(0.0, 0.0, 0.0),
        sample_out=[np.zeros(3) for _ in range(4)])
    assert n_alt == 3
    return a


def _vfo_batch(c, a):
    return c.vfo_batch(*_head(a), _ptr(a["vh"]), a["flags"])


def _vfo_worklist(c, a):
    n = _native()
    segs = None if a["segs"] is None else (n.Segment * len(a["segs"]))(*a["segs"])
    return c._lib.prhf_vfo_worklist_f64(c._h, *_head(a)[:10], _ptr(a["mult"]), a["mult_len"], segs, a["n_segs"], _ptr(a["vh"]),
                                        a["flags"])


def _vfo_residual(c, a):
    return c.vfo_residual(*_head(a), _ptr(a["vh_obs"]), _ptr(a["vh"]), _ptr(a["residual"]), _ptr(a["cost"]), a["flags"])


def _vfo_residual_many(c, a):
    return c.vfo_residual_many(*_head(a), _ptr(a["many_obs"]), a["n_iono"], _ptr(a["ion"]), _ptr(a["vh"]), _ptr(a["residual"]),
                               _ptr(a["many_cost"]), _ptr(a["best"]), _ptr(a["best_cost"]), a["flags"])


def _residual(c, a):
    return c.residual(_ptr(a["vh_model"]), _ptr(a["vh_obs"]), a["n_prof"], a["n_freq"], _ptr(a["residual"]), _ptr(a["cost"]),
                      a["flags"])


def _residual_many(c, a):
    return c.residual_many(_ptr(a["vh_model"]), a["n_prof"], _ptr(a["many_obs"]), a["n_iono"], a["n_freq"], _ptr(a["ion"]),
                           _ptr(a["residual"]), _ptr(a["many_cost"]), _ptr(a["best"]), _ptr(a["best_cost"]), a["flags"])


def _mu_mup(c, a):
    return c.mu_mup(_ptr(a["X"]), _ptr(a["Y"]), _ptr(a["psi"]), a["n"], a["mode"], _ptr(a["mu"]), _ptr(a["mup"]), a["flags"])


def _find_vh(c, a):
    return c.find_vh(_ptr(a["X"]), _ptr(a["Y"]), _ptr(a["psi"]), _ptr(a["dh"]), a["n_rows"], a["n_cols"], a["alt_min"], a["mode"],
                     _ptr(a["find_out"]), a["flags"])


def _regrid(c, a):
    return c.regrid(_ptr(a["freq_hz"]), a["n_freq"], _ptr(a["den1"]), _ptr(a["bmag1"]), _ptr(a["bpsi1"]), _ptr(a["alt"]), a["n_alt"],
                    _ptr(a["mult"]), a["n_points"], a["mode"], [_ptr(o) for o in a["regrid_out"]], a["flags"])


def _field_pack(c, a):
    rc = c.field_pack(_ptr(a["field_mu"]), _ptr(a["field_mup"]), a["n_fields"], a["n0"], a["n1"], _ptr(a["axis0"]), _ptr(a["axis1"]),
                      a["edge_order"], _ptr(a["records"]), a["flags"])
    if rc == _native().OK:                     # (records live on the device in every flag combination)
        a["rec_host"][...] = a["records"].cpu().numpy()
    return rc


def _field_sample(c, a):
    return c.field_sample(_ptr(a["records"]), a["n_fields"], a["n0"], a["n1"], _ptr(a["axis0"]), _ptr(a["axis1"]), _ptr(a["p0"]),
                          _ptr(a["p1"]), _ptr(a["field_index"]), a["n_samples"], a["fills"], [_ptr(o) for o in a["sample_out"]],
                          a["flags"])


def _regrid_without(i):
    outs = _base_regrid_out()
    outs[i] = None
    return outs


def _base_regrid_out():
    return [np.zeros((3, 16)) for _ in range(7)] + [np.zeros((3, 16), dtype=np.int64)]


# check_arguments of run(): context, arrays, [the residual stage's arrays], shape, level limit, n_freq, strides, [segment
# count], flags, ASYNC, the grid; then plan_launch's validate_work_list (mode, n_points, the slices)
def _run_cases():
    return [
        (dict(null_ctx=True), "EINVAL", "null context"),
        (dict(freq=None), "EINVAL", "null array pointer"),
        (dict(den=None), "EINVAL", "null array pointer"),
        (dict(bmag=None), "EINVAL", "null array pointer"),
        (dict(bpsi=None), "EINVAL", "null array pointer"),
        (dict(alt=None), "EINVAL", "null array pointer"),
        (dict(mult=None), "EINVAL", "null array pointer"),
        (dict(n_freq=0), "EINVAL", "bad shape"),
        (dict(n_prof=-1), "EINVAL", "bad shape"),
        (dict(n_alt=0), "EINVAL", "bad shape"),
        (dict(n_alt=1 << 40, prof_stride=1 << 40), "EINVAL", "exceeds the limit of 65535 levels"),
        (dict(n_alt=65536, prof_stride=65536), "EINVAL", "n_alt 65536 exceeds the limit"),
        (dict(prof_stride=2), "EINVAL", "row stride shorter than a row"),
        (dict(alt_stride=2), "EINVAL", "row stride shorter than a row"),
        (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
        (dict(flags=ASYNC), "EINVAL", "PRHF_FLAG_ASYNC needs device pointers"),
        (dict(flags=ASYNC | GRID_STABLE | SHARED_FIELD), "EINVAL", "PRHF_FLAG_ASYNC needs device pointers"),
        (dict(mult=_down_mult()), "EINVAL", "multiplier[5] decreases: the stretched grid must be non-decreasing"),
        # two at once
        (dict(null_ctx=True, den=None), "EINVAL", "null context"),
        (dict(den=None, n_alt=0), "EINVAL", "null array pointer"),
        (dict(n_alt=0, prof_stride=-1), "EINVAL", "bad shape"),
        (dict(n_alt=1 << 40, prof_stride=2), "EINVAL", "exceeds the limit of"),
        (dict(prof_stride=2, flags=BAD_FLAG), "EINVAL", "row stride"),
        (dict(flags=BAD_FLAG | ASYNC), "EINVAL", "unknown flag bits"),
        (dict(flags=ASYNC, mult=_down_mult()), "EINVAL", "PRHF_FLAG_ASYNC"),
    ]


_RUN_FREQ = [                                    # (the many-ionogram entry has a limit of its own in front)
    (dict(n_freq=(1 << 20) + 1), "EINVAL", "n_freq too large"),
    (dict(n_alt=1 << 40, prof_stride=1 << 40, n_freq=(1 << 20) + 1), "EINVAL", "exceeds the limit of"),
    (dict(n_freq=(1 << 20) + 1, prof_stride=2), "EINVAL", "n_freq too large"),
]
def _whole_batch_cases():                       # validate_work_list on the one slice of a call on the whole batch
    return [
        (dict(mode=7), "EINVAL", "mode must be 'O' or 'X'"),
        (dict(n_points=0), "EINVAL", "n_points must be >= 1"),
        (dict(mult=_down_mult(), mode=7), "EINVAL", "multiplier[5] decreases"),
        (dict(mode=7, n_points=0), "EINVAL", "mode must be"),
    ]


def _seg(*v):
    return _native().Segment(*v)


def _worklist_cases():
    n = _native()
    return [
        (dict(segs=None), "EINVAL", "null array pointer"),
        (dict(n_segs=0), "EINVAL", "1..8 segments per launch"),
        (dict(segs=[_seg(0, 2, n.MODE_O, 16, 0, 0)] * 9, n_segs=9), "EINVAL", "1..8 segments per launch"),
        (dict(segs=[_seg(0, 3, n.MODE_O, 16, 0, 0)]), "EINVAL", "segment 0: profile range outside [0, n_prof]"),
        (dict(segs=[_seg(1, 0, n.MODE_O, 16, 0, 0)]), "EINVAL", "segment 0: profile range outside [0, n_prof]"),
        (dict(segs=[_seg(0, 2, 7, 16, 0, 0)]), "EINVAL", "mode must be 'O' or 'X'"),
        (dict(segs=[_seg(0, 2, n.MODE_O, 0, 0, 0)]), "EINVAL", "n_points must be >= 1"),
        (dict(segs=[_seg(0, 2, n.MODE_O, 16, 1, 0)]), "EINVAL", "segment 0: multiplier range outside the array"),
        (dict(mult_len=15), "EINVAL", "segment 0: multiplier range outside the array"),
        (dict(segs=[_seg(0, 2, n.MODE_O, 16, 0, 1)]), "EINVAL", "segment 0: output offset must be a non-negative multiple of n_freq"),
        (dict(segs=[_seg(0, 1, n.MODE_O, 16, 0, 0), _seg(1, 2, n.MODE_X, 16, 0, 0)], n_segs=2), "EINVAL",
         "segments 0 and 1 write the same output rows"),
        (dict(segs=None, n_freq=0), "EINVAL", "null array pointer"),
        (dict(prof_stride=2, n_segs=0), "EINVAL", "row stride"),
        (dict(n_segs=0, flags=BAD_FLAG), "EINVAL", "1..8 segments per launch"),
        (dict(flags=BAD_FLAG, segs=[_seg(0, 3, n.MODE_O, 16, 0, 0)]), "EINVAL", "unknown flag bits"),
        (dict(mult=_down_mult(), segs=[_seg(0, 3, n.MODE_O, 16, 0, 0)]), "EINVAL", "multiplier[5] decreases"),
        (dict(segs=[_seg(0, 3, 7, 16, 0, 0)]), "EINVAL", "segment 0: profile range"),
    ]


# check_many: arrays, shape, the grid's limit, 2^31, shared candidates, 2^36 pairs; host buffers: a finite grid (the fused
# entry), ionogram_of_row in range and non-decreasing.  n_rows is n_prof here.
_MANY = [
    (dict(many_obs=None), "EINVAL", "null array pointer"),
    (dict(many_cost=None), "EINVAL", "null array pointer"),
    (dict(best=None), "EINVAL", "null array pointer"),
    (dict(best_cost=None), "EINVAL", "null array pointer"),
    (dict(n_prof=-1), "EINVAL", "bad shape"),
    (dict(n_iono=0), "EINVAL", "bad shape"),
    (dict(n_freq=0), "EINVAL", "bad shape"),
    (dict(n_freq=MANY_MAX_FREQ + 1), "EINVAL", "n_freq 4097 exceeds the many-ionogram limit of 4096 grid frequencies"),
    (dict(n_prof=BIG), "EINVAL", "bad shape: more than 2^31 - 1 rows or ionograms"),
    (dict(n_iono=BIG), "EINVAL", "bad shape: more than 2^31 - 1 rows or ionograms"),
    (dict(ion=None), "EINVAL", "shared candidates have no dense residual output"),
    (dict(ion=None, residual=None, n_prof=1 << 30, n_iono=65), "EINVAL", "bad shape: more than 2^36 (ionogram, candidate) pairs"),
    (dict(ion=I32(0, 2)), "EINVAL", "ionogram_of_row[1] outside [0, n_iono)"),
    (dict(ion=I32(-1, 0)), "EINVAL", "ionogram_of_row[0] outside [0, n_iono)"),
    (dict(ion=I32(1, 0)), "EINVAL", "ionogram_of_row[1] decreases: the rows of an ionogram must be contiguous"),
    (dict(null_ctx=True), "EINVAL", "null context"),
    # two at once: the arrays and shapes of check_many come before the null context
    (dict(null_ctx=True, many_obs=None), "EINVAL", "null array pointer"),
    (dict(null_ctx=True, ion=I32(1, 0)), "EINVAL", "ionogram_of_row[1] decreases"),
    (dict(best=None, n_iono=0), "EINVAL", "null array pointer"),
    (dict(n_iono=0, n_freq=MANY_MAX_FREQ + 1), "EINVAL", "bad shape"),
    (dict(n_freq=MANY_MAX_FREQ + 1, n_prof=BIG), "EINVAL", "exceeds the many-ionogram limit"),
    (dict(n_prof=BIG, ion=None), "EINVAL", "more than 2^31 - 1"),
    (dict(ion=I32(0, 2), flags=BAD_FLAG), "EINVAL", "ionogram_of_row[1] outside"),
    (dict(null_ctx=True, flags=BAD_FLAG), "EINVAL", "null context"),
]

_STAGE_FLAGS = [                                 # the stage ops take PRHF_FLAG_DEVICE_PTRS only
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
    (dict(flags=ASYNC), "EINVAL", "unknown flag bits"),
    (dict(flags=GRID_STABLE), "EINVAL", "unknown flag bits"),
]
_BAD_AXIS = F64(0.0, 2.0, 1.0, 3.0)
_FIELD_SHAPE = [                                 # check_field_shape: the axes, the shape, axis 0, axis 1
    (dict(axis0=None), "EINVAL", "null array pointer"),
    (dict(axis1=None), "EINVAL", "null array pointer"),
    (dict(n_fields=0), "EINVAL", "bad shape (the two axes hold at most 8000 values together)"),
    (dict(n0=0), "EINVAL", "bad shape (the two axes hold at most"),
    (dict(n1=0), "EINVAL", "bad shape (the two axes hold at most"),
    (dict(n0=4000, n1=4001), "EINVAL", "bad shape (the two axes hold at most"),
    (dict(n_fields=(1 << 24) + 1), "EINVAL", "bad shape (the two axes hold at most"),
    (dict(n0=1), "EINVAL", "axis 0 needs at least"),
    (dict(n1=1), "EINVAL", "axis 1 needs at least"),
    (dict(axis0=_BAD_AXIS), "EINVAL", "axis 0 must be strictly increasing"),
    (dict(axis1=_BAD_AXIS), "EINVAL", "axis 1 must be strictly increasing"),
    (dict(axis0=F64(0.0, 1.0, float("nan"), 3.0)), "EINVAL", "axis 0 must be strictly increasing"),
    (dict(flags=BAD_FLAG, axis0=None), "EINVAL", "unknown flag bits"),
    (dict(axis1=None, n_fields=0), "EINVAL", "null array pointer"),
    (dict(n_fields=0, axis0=_BAD_AXIS), "EINVAL", "bad shape"),
    (dict(axis0=_BAD_AXIS, axis1=_BAD_AXIS), "EINVAL", "axis 0 must be"),
]


def _entry_points():
    _RUN, _WHOLE_BATCH = _run_cases(), _whole_batch_cases()
    return {
        # prhf_vfo_batch_f64: a call that a check part refuses never takes the slab route (the last three cases: a batch
        # large enough for it)
        "vfo_batch": (_vfo_batch, _RUN + _RUN_FREQ + _WHOLE_BATCH + [
            (dict(vh=None), "EINVAL", "null array pointer"),
            (dict(vh=None, n_freq=0), "EINVAL", "null array pointer"),
            (dict(n_prof=1 << 22, den=None), "EINVAL", "null array pointer"),
            (dict(n_prof=1 << 22, prof_stride=2, flags=BAD_FLAG), "EINVAL", "row stride"),
            (dict(n_prof=1 << 22, mode=7, flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
        ], "vh"),
        "vfo_worklist": (_vfo_worklist, _RUN + _RUN_FREQ + _worklist_cases() + [
            (dict(vh=None), "EINVAL", "null array pointer"),
        ], "vh"),
        # prhf_vfo_residual_f64: vh_out may be null; the observed trace and one of residual / cost may not
        "vfo_residual": (_vfo_residual, _RUN + _RUN_FREQ + _WHOLE_BATCH + [
            (dict(vh_obs=None), "EINVAL", "null array pointer"),
            (dict(residual=None, cost=None), "EINVAL", "null array pointer"),
            (dict(vh_obs=None, n_freq=0), "EINVAL", "null array pointer"),
            (dict(null_ctx=True, vh_obs=None), "EINVAL", "null context"),
        ], "vh"),
        # prhf_vfo_residual_many_f64: the grid and check_many first, then run()
        "vfo_residual_many": (_vfo_residual_many, [ch for ch in _RUN if "n_freq" not in ch[0] and "null_ctx" not in ch[0]] + _MANY
                              + _WHOLE_BATCH + [
            (dict(freq=F64(1.0, float("inf"), 10.0)), "EINVAL", "freq_mhz[1] is not finite: the common grid must be"),
            (dict(freq=F64(float("nan"), 2.0, 10.0), ion=I32(1, 0)), "EINVAL", "freq_mhz[0] is not finite"),
            (dict(freq=None, many_obs=None, null_ctx=True), "EINVAL", "null array pointer"),
            (dict(ion=I32(1, 0), den=None), "EINVAL", "ionogram_of_row[1] decreases"),
        ], "vh"),
        # prhf_residual_f64
        "residual": (_residual, [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(vh_model=None), "EINVAL", "null array pointer"),
            (dict(vh_obs=None), "EINVAL", "null array pointer"),
            (dict(residual=None, cost=None), "EINVAL", "null array pointer"),
            (dict(n_prof=-1), "EINVAL", "bad shape"),
            (dict(n_freq=0), "EINVAL", "bad shape"),
            (dict(n_freq=(1 << 20) + 1), "EINVAL", "bad shape"),
            (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
            (dict(flags=SHARED_FIELD), "EINVAL", "unknown flag bits"),
            (dict(flags=ASYNC), "EINVAL", "PRHF_FLAG_ASYNC and PRHF_FLAG_GRID_STABLE need device pointers"),
            (dict(flags=GRID_STABLE), "EINVAL", "PRHF_FLAG_ASYNC and PRHF_FLAG_GRID_STABLE need device pointers"),
            (dict(n_prof=0), "OK", ""),
            (dict(null_ctx=True, vh_model=None), "EINVAL", "null context"),
            (dict(vh_obs=None, n_freq=0), "EINVAL", "null array pointer"),
            (dict(n_freq=0, flags=BAD_FLAG), "EINVAL", "bad shape"),
            (dict(flags=BAD_FLAG | ASYNC), "EINVAL", "unknown flag bits"),
            (dict(n_prof=0, flags=ASYNC), "EINVAL", "need device pointers"),
        ], "residual"),
        # prhf_residual_many_f64: the model rows, check_many, then context and flags
        "residual_many": (_residual_many, _MANY + [
            (dict(vh_model=None), "EINVAL", "null array pointer"),
            (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
            (dict(flags=GRID_STABLE), "EINVAL", "unknown flag bits"),
            (dict(flags=ASYNC), "EINVAL", "PRHF_FLAG_ASYNC needs device pointers"),
            (dict(vh_model=None, null_ctx=True), "EINVAL", "null array pointer"),
            (dict(flags=BAD_FLAG | ASYNC), "EINVAL", "unknown flag bits"),
        ], "best_cost"),
        "mu_mup": (_mu_mup, _STAGE_FLAGS + [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(X=None), "EINVAL", "null array pointer"),
            (dict(Y=None), "EINVAL", "null array pointer"),
            (dict(psi=None), "EINVAL", "null array pointer"),
            (dict(mu=None), "EINVAL", "null array pointer"),
            (dict(mup=None), "EINVAL", "null array pointer"),
            (dict(n=-1), "EINVAL", "bad shape"),
            (dict(mode=7), "EINVAL", "Mode must be O or X"),
            (dict(n=0), "OK", ""),
            (dict(null_ctx=True, X=None), "EINVAL", "null context"),
            (dict(mup=None, n=-1), "EINVAL", "null array pointer"),
            (dict(n=-1, mode=7), "EINVAL", "bad shape"),
            (dict(mode=7, flags=BAD_FLAG), "EINVAL", "Mode must be O or X"),
            (dict(n=0, flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
        ], "mu"),
        "find_vh": (_find_vh, _STAGE_FLAGS + [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(X=None), "EINVAL", "null array pointer"),
            (dict(dh=None), "EINVAL", "null array pointer"),
            (dict(find_out=None), "EINVAL", "null array pointer"),
            (dict(n_rows=-1), "EINVAL", "bad shape"),
            (dict(n_cols=-1), "EINVAL", "bad shape"),
            (dict(mode=7), "EINVAL", "Mode must be O or X"),
            (dict(n_rows=0), "OK", ""),
            (dict(null_ctx=True, dh=None), "EINVAL", "null context"),
            (dict(dh=None, n_cols=-1), "EINVAL", "null array pointer"),
            (dict(n_cols=-1, mode=7), "EINVAL", "bad shape"),
            (dict(mode=7, flags=BAD_FLAG), "EINVAL", "Mode must be O or X"),
            (dict(n_rows=0, flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
        ], "find_out"),
        "regrid": (_regrid, _STAGE_FLAGS + [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(freq_hz=None), "EINVAL", "null array pointer"),
            (dict(den1=None), "EINVAL", "null array pointer"),
            (dict(bmag1=None), "EINVAL", "null array pointer"),
            (dict(bpsi1=None), "EINVAL", "null array pointer"),
            (dict(alt=None), "EINVAL", "null array pointer"),
            (dict(mult=None), "EINVAL", "null array pointer"),
        ] + [(dict(regrid_out=_regrid_without(i)), "EINVAL", "null array pointer") for i in range(8)] + [
            (dict(n_freq=0), "EINVAL", "bad shape"),
            (dict(n_alt=0), "EINVAL", "bad shape"),
            (dict(n_alt=65536), "EINVAL", "bad shape"),
            (dict(n_points=0), "EINVAL", "bad shape"),
            (dict(mode=7), "EINVAL", "mode must be 'O' or 'X'"),
            (dict(null_ctx=True, den1=None), "EINVAL", "null context"),
            (dict(regrid_out=_regrid_without(7), n_alt=65536), "EINVAL", "null array pointer"),
            (dict(n_alt=65536, mode=7), "EINVAL", "bad shape"),
            (dict(mode=7, flags=BAD_FLAG), "EINVAL", "mode must be"),
        ], lambda a: a["regrid_out"][0]),
        # prhf_field_pack_f64: context, arrays, edge_order, flags, then the field's shape (axes of edge_order + 1 values)
        "field_pack": (_field_pack, _STAGE_FLAGS + _FIELD_SHAPE + [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(field_mu=None), "EINVAL", "null array pointer"),
            (dict(field_mup=None), "EINVAL", "null array pointer"),
            (dict(records=None), "EINVAL", "null array pointer"),
            (dict(edge_order=0), "EINVAL", "edge_order is 1 or 2"),
            (dict(edge_order=3), "EINVAL", "edge_order is 1 or 2"),
            (dict(n0=2), "EINVAL", "axis 0 needs at least 3 values"),
            (dict(n0=2, edge_order=1), "OK", ""),
            (dict(null_ctx=True, records=None), "EINVAL", "null context"),
            (dict(records=None, edge_order=3), "EINVAL", "null array pointer"),
            (dict(edge_order=3, flags=BAD_FLAG), "EINVAL", "edge_order is"),
        ], "rec_host"),
        # prhf_field_sample_f64: context, arrays, an output, n, flags, the field's shape, field_index, then n == 0
        "field_sample": (_field_sample, _STAGE_FLAGS + _FIELD_SHAPE + [
            (dict(null_ctx=True), "EINVAL", "null context"),
            (dict(records=None), "EINVAL", "null array pointer"),
            (dict(p0=None), "EINVAL", "null array pointer"),
            (dict(p1=None), "EINVAL", "null array pointer"),
            (dict(sample_out=[None] * 4), "EINVAL", "no output asked for"),
            (dict(n_samples=-1), "EINVAL", "bad shape"),
            (dict(field_index=I64(0, 2, 0)), "EINVAL", "field_index[1] outside [0, n_fields)"),
            (dict(field_index=I64(-1, 0, 0)), "EINVAL", "field_index[0] outside [0, n_fields)"),
            (dict(n_samples=0), "OK", ""),
            (dict(field_index=None), "OK", ""),
            (dict(null_ctx=True, p0=None), "EINVAL", "null context"),
            (dict(p1=None, sample_out=[None] * 4), "EINVAL", "null array pointer"),
            (dict(sample_out=[None] * 4, n_samples=-1), "EINVAL", "no output asked for"),
            (dict(n_samples=-1, flags=BAD_FLAG), "EINVAL", "bad shape"),
            (dict(axis0=_BAD_AXIS, field_index=I64(0, 2, 0)), "EINVAL", "axis 0 must be"),
            (dict(n_samples=0, field_index=I64(0, 2, 0)), "OK", ""),
        ], lambda a: a["sample_out"][0]),
    }


ENTRY_POINTS = ["vfo_batch", "vfo_worklist", "vfo_residual", "vfo_residual_many", "residual", "residual_many", "mu_mup", "find_vh",
                "regrid", "field_pack", "field_sample"]


@pytest.fixture(scope="module")
def base():
    return _base()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_operator_entry_point_rejections(name, ctx, null_ctx, base):      # noqa: F811
    n = _native()
    call, cases, out = _entry_points()[name]
    first = out if callable(out) else (lambda a: a[out])
    _run(call, dict(base), [(ch, getattr(n, rc), text) for ch, rc, text in cases], ctx, null_ctx, first)
