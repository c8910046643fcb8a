"""The host-side half of option pair_plan, without a GPU: the option table of prhf_plan.h knows it, the
launch planner leaves it off for tall and chunked slices (slice_plans_pairs - the very code prhf_api.cpp compiles), and
a library that lacks prhf_pair_plan_counters is refused when it is loaded."""

import os
import subprocess
import sys

from conftest import REPO

PLANNER = r"""
#include <cstdio>
#include <cstring>
#include "prhf_plan.h"

static prhf::SegDev slice(long long profiles, long long n_freq, int n_points, const Knobs& kn) {
    prhf::SegDev s;
    std::memset(&s, 0, sizeof s);
    s.prof_begin = 0; s.prof_end = profiles; s.mode = PRHF_KMODE_X; s.n_points = n_points; s.tier = 1; s.lean = 1;
    s.thread_scan = 1;
    plan_slice(s, n_freq, 512, kn);
    s.sp_off = s.chunks == 1 ? 123456 : 0;      // (the strided table has a piece for whole pairs only)
    return s;
}
#define CHECK(x) do { if (!(x)) { std::printf("failed: %s\n", #x); return 1; } } while (0)

int main() {
    Knobs kn;
    const KnobName* plan = nullptr;
    const KnobName* cap = nullptr;
    for (const KnobName& k : kKnobNames) {
        if (!std::strcmp(k.name, "pair_plan")) plan = &k;
        if (!std::strcmp(k.name, "pair_plan_cap")) cap = &k;
    }
    CHECK(plan && plan->lo == 0 && plan->hi == 1 && kn.*(plan->field) == 1);
    CHECK(cap && cap->lo == 0 && kn.*(cap->field) == 0);
    const long long levels = 620;
    prhf::SegDev s = slice(12500, 256, 20000, kn);
    CHECK(s.chunks == 1 && s.slots == 0);
    CHECK(slice_plans_pairs(s, false, 256, levels, kn));
    CHECK(!slice_plans_pairs(s, true, 256, levels, kn));                 // tall: staged in global memory
    Knobs off = kn;
    off.pair_plan = 0;
    CHECK(!slice_plans_pairs(s, false, 256, levels, off));
    Knobs all = kn;
    all.no_candidates = 1;
    CHECK(!slice_plans_pairs(s, false, 256, levels, all));              // no candidate list, no settled heights
    CHECK(!slice_plans_pairs(s, false, 600, levels, kn));               // more than one round of frequencies
    CHECK(!slice_plans_pairs(s, false, 256, 200, kn));                  // heights would not fit the staged arrays
    prhf::SegDev one = slice(1, 174, 20000, kn);                        // one profile: chunked
    CHECK(one.chunks > 1 || one.slots > 0);
    one.sp_off = 123456;
    CHECK(!slice_plans_pairs(one, false, 174, levels, kn));
    prhf::SegDev wide = slice(12500, 256, 65536, kn);                   // the plan's fields are 16 bits wide
    CHECK(!slice_plans_pairs(wide, false, 256, levels, kn));
    prhf::SegDev shorter = slice(12500, 256, 8191, kn);
    CHECK(!slice_plans_pairs(shorter, false, 256, levels, kn));
    prhf::SegDev o = s;
    o.mode = PRHF_KMODE_O; o.tier = 0;
    CHECK(!slice_plans_pairs(o, false, 256, levels, kn));
    prhf::SegDev none = s;
    none.sp_off = 0;                                                    // strided_top = 0, or no room for the piece
    CHECK(!slice_plans_pairs(none, false, 256, levels, kn));
    std::printf("pair_plan_host: ok\n");
    return 0;
}
"""


def test_option_table_and_planner(tmp_path):
    src, exe = tmp_path / "pair_plan_host.cpp", tmp_path / "pair_plan_host"
    src.write_text(PLANNER)
    inc = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__"]          # prhf_kernels.h includes hip_runtime_api.h for its launch prototypes (types only)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", *inc, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "pair_plan_host: ok" in run.stdout, run.stdout + run.stderr


def test_a_library_without_the_counter_call_is_refused(tmp_path):
    """Every symbol of the binding but prhf_pair_plan_counters, the right ABI number: the loader must name what is missing."""
    from pyrayhf_amd import _native
    names = [n for n in _native.exported_symbols() if n not in ("prhf_pair_plan_counters", "prhf_abi_version")]
    assert "prhf_pair_plan_counters" in _native.exported_symbols()
    stub = tmp_path / "stub.c"
    stub.write_text("".join(f"int {n}(void) {{ return 0; }}\n" for n in names) +
                    f"int prhf_abi_version(void) {{ return {_native.ABI_VERSION}; }}\n")
    lib = tmp_path / "libprhf.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(stub), "-o", str(lib)], check=True)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from pyrayhf_amd import _native\n"
            "try:\n"
            "    _native.load()\n"
            "    print('LOADED')\n"
            "except _native.NativeLibraryError as exc:\n"
            "    print('REFUSED', 'prhf_pair_plan_counters' in str(exc))\n" % REPO)
    env = dict(os.environ, PRHF_LIB=str(lib), PRHF_NO_TORCH_PRELOAD="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert "REFUSED True" in out.stdout, out.stdout + out.stderr
