"""The launch planner (pyrayhf_amd/csrc/prhf_plan.h, plan_launch - the very code prhf_api.cpp compiles) without a GPU:
the structural invariants of a plan over a table of shapes, two anchors that follow from plan_slice by hand, what each
launch-shaping option changes (tests/devtools/launch_plan_host.cpp), and the dispatches of the commit before plan_launch
existed, recorded on an MI355X under `rocprofv3 --kernel-trace` (profiles/launch_plan_parent.jsonl), which the plan
must reproduce kernel by kernel."""

import json
import os
import subprocess

import pytest

from conftest import REPO

PARENT = os.path.join(REPO, "profiles", "launch_plan_parent.jsonl")
REFACTOR = os.path.join(REPO, "profiles", "launch_plan_refactor.jsonl")
# kernels of a recorded call that the plan does not place: the pair table and its strided pieces are cached per grid
# (a later shape on the same grid does not build them again), the peak pre-pass belongs to run()'s tall decision
NOT_PLANNED = ("grid_pairs_kernel", "grid_strided_kernel", "peak_levels_kernel")
# (The profiler's LDS column holds a kernel's static allocation only - 512 bytes for every kernel here - so the two
#  recordings are compared on it, and the dynamic bytes of the plan are pinned by the invariants instead: each launch's
#  LDS equals the kernel header's formula for its levels, threads and queue.)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_host"
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]          # prhf_kernels.h includes hip_runtime_api.h for its launch prototypes (types only)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", *inc, os.path.join(REPO, "tests", "devtools", "launch_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_invariants_anchors_and_options(planner):
    run = subprocess.run([planner, "check"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "launch_plan_host: ok" in run.stdout, run.stdout + run.stderr


def records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_both_builds_dispatched_the_same():
    """The two recordings, kernel by kernel: name, workgroups, workgroup size, LDS bytes."""
    parent, refactor = records(PARENT), records(REFACTOR)
    assert [r["name"] for r in parent] == [r["name"] for r in refactor] and len(parent) >= 10
    for a, b in zip(parent, refactor):
        assert a["dispatches"] == b["dispatches"], a["name"]


def test_plan_reproduces_the_recorded_dispatches(planner):
    recs = records(PARENT)
    lines = []
    for r in recs:
        segs = " ".join(f"{b} {e} {mode} {n}" for b, e, mode, n in r["segments"])
        lines.append(f"{r['name']} {r['n_prof']} {r['n_freq']} {r['n_alt']} {r['lds_levels']} {r['tall']} {len(r['segments'])} {segs}")
    run = subprocess.run([planner, "predict"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    planned = {r["name"]: [] for r in recs}
    for line in run.stdout.splitlines():
        name, kernel, grid, threads, lds = line.split()
        planned[name].append((kernel, int(grid), int(threads), int(lds)))
    for r in recs:
        recorded = [d for d in r["dispatches"] if not d[0].startswith(NOT_PLANNED)]
        got = planned[r["name"]]
        assert [d[0] for d in recorded] == [p[0] for p in got], (r["name"], recorded, got)
        for (kernel, grid, threads, _), (_, p_grid, p_threads, _) in zip(recorded, got):
            if kernel.startswith(("freq_table_kernel", "short_order_kernel")):
                continue                       # (the plan says which of the two makes the table; its geometry is the launcher's)
            assert (grid, threads) == (p_grid, p_threads), (r["name"], kernel, grid, threads, p_grid, p_threads)
