"""plan_launch's decision for the streaming form of the persistent launch (pyrayhf_amd/csrc/prhf_plan.h, LaunchPlan::stream;
options stream_blocks, stream_grid) without a GPU: tests/devtools/stream_plan_host.cpp holds the decision to its
conditions - the config-4 shard and config 4 in full take the form; config 3, config 5, config 2, O mode, a tall column,
700 levels (one slot fits, two do not) and stream_blocks = 0 keep the general kernel; stream_grid caps the workgroups.
Built with AddressSanitizer + UndefinedBehaviorSanitizer, as the planner is in tests/test_sanitizers_host.py."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_decision_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]          # prhf_kernels.h includes hip_runtime_api.h for its launch prototypes (types only)
    exe = tmp_path / "stream_plan_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", *san, *inc, os.path.join(REPO, "tests", "devtools", "stream_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe), "check"], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "stream_plan_host: ok" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
