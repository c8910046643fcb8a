#!/usr/bin/env python3
"""Two builds of the library on the operator, its residual stages and the un-fused stage ops, through the raw Context:
    PRHF_LIB=<build> python tools/ab_operator_drivers.py calls OUT.npz [--host-only]   every output array of one host-buffer
                                                     and one device-pointer call per entry point (small shapes), of the
                                                     single-profile host call (1 x 174, both modes) and of a host batch
                                                     large enough for the slab route
    python tools/ab_operator_drivers.py compare A.npz B.npz                            arrays equal / differing (NaN == NaN)
    python tools/ab_operator_drivers.py dispatch TRACE_DIR OUT.jsonl [--start-order]   a `rocprofv3 --kernel-trace
                                                     --output-format csv -d TRACE_DIR -- ... calls X.npz --host-only` run
                                                     as one line per dispatch, by stream and in start order within it:
                                                     kernel, workgroups, workgroup size, LDS bytes
(profiles/ab_operator_drivers.txt)."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def calls(out_path, host_only):
    import torch
    from pyrayhf_amd import _native as n, library, synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "g1_basic.npz"))
    two = lambda k: np.ascontiguousarray(np.stack([g[k], g[k] * 1.01]), dtype=np.float64)      # noqa: E731
    freq, alt = g["freq"].astype(np.float64), g["alt"].astype(np.float64)
    den, bmag, bpsi, mult = two("den"), two("bmag"), two("bpsi"), np.ascontiguousarray(library._multiplier(16))
    obs, many_obs = np.array([100.0, 110.0, 120.0]), np.array([[100.0, 110.0, 120.0], [105.0, 115.0, 125.0]])
    ion, model = np.array([0, 1], dtype=np.int32), np.array([[101.0, 111.0, 121.0], [104.0, 114.0, 124.0]])
    X, Y = np.tile(np.array([0.1, 0.3, 0.5, 0.7]), (2, 1)), np.full((2, 4), 0.3)
    psi, dh, axis = np.full((2, 4), 60.0), np.full((2, 4), 1.0), np.array([0.0, 1.0, 2.0, 3.0])
    fmu = np.linspace(0.5, 0.95, 32).reshape(2, 4, 4)
    fmup = 1.0 / fmu
    p0, p1, fidx = np.array([0.5, 1.5, 2.5]), np.array([2.5, 1.5, 0.5]), np.array([0, 1, 0], dtype=np.int64)
    seg = [n.Segment(0, 1, n.MODE_O, 16, 0, 0), n.Segment(1, 2, n.MODE_X, 16, 0, 3)]
    results = {}

    def run(tag, ctx, flags, to, z):
        """One call per entry point: `to` puts an input where the call reads it, `z` makes an output there."""
        P = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v.data_ptr())      # noqa: E731
        back = lambda v: v if isinstance(v, np.ndarray) else v.cpu().numpy()                                      # noqa: E731
        d = {k: to(v) for k, v in dict(freq=freq, den=den, bmag=bmag, bpsi=bpsi, alt=alt, mult=mult, obs=obs, many_obs=many_obs,
                                       ion=ion, model=model, X=X, Y=Y, psi=psi, dh=dh, fmu=fmu, fmup=fmup, p0=p0, p1=p1, fidx=fidx,
                                       freq_hz=freq * 1e6, den1=den[0].copy(), bmag1=bmag[0].copy(), bpsi1=bpsi[0].copy()).items()}
        head = (P(d["freq"]), 3, P(d["den"]), P(d["bmag"]), P(d["bpsi"]), P(d["alt"]), 2, 3, 3, 0, P(d["mult"]), 16)

        def keep(name, rc, **outs):
            n.raise_for(rc)
            n.raise_for(ctx.sync())
            torch.cuda.synchronize()
            for k, v in outs.items():
                results[f"{tag}.{name}.{k}"] = back(v).copy()

        for mode in (n.MODE_O, n.MODE_X):
            vh = z((2, 3))
            keep(f"vfo_batch{mode}", ctx.vfo_batch(*head, mode, P(vh), flags), vh=vh)
        vh = z((2, 3))
        keep("vfo_worklist", ctx.vfo_worklist(*head[:11], 16, seg, P(vh), flags), vh=vh)
        vh, res, cost = z((2, 3)), z((2, 3)), z(2)
        keep("vfo_residual", ctx.vfo_residual(*head, n.MODE_O, P(d["obs"]), P(vh), P(res), P(cost), flags), vh=vh, res=res, cost=cost)
        vh, res, cost, best, bc = z((2, 3)), z((2, 3)), z(2), z(2, np.int64), z(2)
        keep("vfo_residual_many", ctx.vfo_residual_many(*head, n.MODE_O, P(d["many_obs"]), 2, P(d["ion"]), P(vh), P(res), P(cost),
                                                        P(best), P(bc), flags), vh=vh, res=res, cost=cost, best=best, bc=bc)
        cost, best, bc = z((2, 2)), z(2, np.int64), z(2)                   # shared candidates: no ionogram_of_row, no residual
        keep("vfo_residual_shared", ctx.vfo_residual_many(*head, n.MODE_O, P(d["many_obs"]), 2, None, None, None, P(cost), P(best),
                                                          P(bc), flags), cost=cost, best=best, bc=bc)
        res, cost = z((2, 3)), z(2)
        keep("residual", ctx.residual(P(d["model"]), P(d["obs"]), 2, 3, P(res), P(cost), flags), res=res, cost=cost)
        res, cost, best, bc = z((2, 3)), z(2), z(2, np.int64), z(2)
        keep("residual_many", ctx.residual_many(P(d["model"]), 2, P(d["many_obs"]), 2, 3, P(d["ion"]), P(res), P(cost), P(best), P(bc),
                                                flags), res=res, cost=cost, best=best, bc=bc)
        mu, mup = z(8), z(8)
        keep("mu_mup", ctx.mu_mup(P(d["X"]), P(d["Y"]), P(d["psi"]), 8, n.MODE_O, P(mu), P(mup), flags), mu=mu, mup=mup)
        fv = z(2)
        keep("find_vh", ctx.find_vh(P(d["X"]), P(d["Y"]), P(d["psi"]), P(d["dh"]), 2, 4, 100.0, n.MODE_X, P(fv), flags), vh=fv)
        ro = [z((3, 16)) for _ in range(7)] + [z((3, 16), np.int64)]
        keep("regrid", ctx.regrid(P(d["freq_hz"]), 3, P(d["den1"]), P(d["bmag1"]), P(d["bpsi1"]), P(d["alt"]), 3, P(d["mult"]), 16,
                                  n.MODE_O, [P(o) for o in ro], flags), **{f"out{i}": o for i, o in enumerate(ro)})
        rec = torch.zeros((2, 4, 4, 4), dtype=torch.float64, device="cuda:0")      # (records: device memory in every call)
        keep("field_pack", ctx.field_pack(P(d["fmu"]), P(d["fmup"]), 2, 4, 4, axis.ctypes.data, axis.ctypes.data, 2, P(rec), flags),
             rec=rec)
        so = [z(3) for _ in range(4)]
        keep("field_sample", ctx.field_sample(P(rec), 2, 4, 4, axis.ctypes.data, axis.ctypes.data, P(d["p0"]), P(d["p1"]), P(d["fidx"]),
                                              3, (0.0, 0.0, 0.0), [P(o) for o in so], flags),
             **{f"out{i}": o for i, o in enumerate(so)})

    host = n.host_context(0)
    run("host", host, 0, lambda v: np.ascontiguousarray(v), lambda shape, dt=np.float64: np.full(shape, -7, dtype=dt))
    # the single-profile host call (pack / direct upload, result straight into pinned memory) and a batch in slabs
    alt1, den1, bmag1, bpsi1 = synth.chapman_profiles(1536, 7)
    f174 = synth.sounder_frequencies(1)
    for mode, points in (("O", 200), ("X", 2000)):
        for _ in range(2):                     # (the second call finds the arena idle and sized)
            results[f"host.single_{mode}"] = library.vertical_forward_operator(f174, den1[:1], bmag1[:1], bpsi1[:1], alt1, mode, points,
                                                                               device=0)
    assert den1.shape[0] * den1.shape[1] * 24 >= 16 << 20
    results["host.slabs"] = library.vertical_forward_operator(f174, den1, bmag1, bpsi1, alt1, "O", 200, device=0)
    if not host_only:
        dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).to("cuda:0")                                     # noqa: E731
        zdev = lambda shape, dt=np.float64: torch.full(shape if isinstance(shape, tuple) else (shape,), -7,       # noqa: E731
                                                       dtype=torch.float64 if dt == np.float64 else torch.int64, device="cuda:0")
        run("dev", n.context(0), n.FLAG_DEVICE_PTRS, dev, zdev)
    np.savez(out_path, **results)
    print(json.dumps({"lib": n.LIB_PATH, "arrays": len(results), "host_only": host_only}))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    differ = [k for k in names if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    untouched = [k for k in names if k in a.files and a[k].size and np.all(a[k] == -7)]
    print(json.dumps({"arrays": len(names), "equal": len(names) - len(differ), "differ": differ, "never_written": untouched,
                      "values": int(sum(a[k].size for k in a.files))}))
    return 1 if differ else 0


def dispatch(trace_dir, out_path, start_order):
    """Streams run beside each other (a slab's rows go home on `down_stream` while the next slab's kernels run), so the
    start order across streams is a race; within a stream it is the order of the calls.  Default: by stream, each in start
    order.  --start-order: one list in start order, as the trace has it."""
    found = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for path in found for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: (0 if start_order else int(r["Stream_Id"]), int(r["Start_Timestamp"])))
    with open(out_path, "w") as fp:
        for r in rows:
            size = [int(r[f"Workgroup_Size_{ax}"]) for ax in "XYZ"]
            grid = [int(r[f"Grid_Size_{ax}"]) for ax in "XYZ"]
            line = {"kernel": r["Kernel_Name"], "workgroups": int(np.prod([g // s for g, s in zip(grid, size)])),
                    "workgroup_size": int(np.prod(size)), "lds_bytes": int(r["LDS_Block_Size"])}
            fp.write(json.dumps(line if start_order else dict(stream=int(r["Stream_Id"]), **line)) + "\n")
    print(json.dumps({"dispatches": len(rows), "files": len(found), "order": "start" if start_order else "stream, start"}))


if __name__ == "__main__":
    if sys.argv[1] == "calls":
        calls(sys.argv[2], "--host-only" in sys.argv[3:])
    elif sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif sys.argv[1] == "dispatch":
        dispatch(sys.argv[2], sys.argv[3], "--start-order" in sys.argv[4:])
