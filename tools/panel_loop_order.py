#!/usr/bin/env python
"""Is the panel sum's evaluation loop still compiled with its look-up in flight?  Runs without a GPU.

The loop asks for the next entry's m before it evaluates the entry it has.  That order rests on two pieces of steering
in lean_loop_body (an empty asm with a memory clobber in front of the evaluation; the table's address through a scalar
register), and a compiler that sinks the load to its first use again would change no output, so no test would notice.
This tool cross-compiles prhf_kernels.hip for gfx950 with the Makefile's flags, finds in every X-mode instance of the
loop function the loops that hold the list word's ds_bpermute_b32, the table row's global_load_dwordx4 and v_rsq_f64,
and checks in each: after every buffer_load_dwordx2 (m of the next entry) both v_rsq_f64 of the current entry's
evaluation come before the next wait on the vector-memory counter.  It prints the loops it judged and exits with 1 if
one fails or none is found.

Usage: python tools/panel_loop_order.py [--hipcc /opt/rocm/bin/hipcc] [--keep file.s]
"""

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-mllvm", "-disable-machine-licm"]


def loops_of(body):
    """Innermost-first (label, instructions) of every loop of one function: a label and a branch back to it."""
    labels = {m.group(1): j for j, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    for j, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < j:
            yield m.group(1), [s.strip() for s in body[labels[m.group(1)]:j + 1] if re.match(r"\s+[a-z]", s)]


def in_flight(ins):
    """After every buffer_load_dwordx2, cyclically, two v_rsq_f64 stand before the next s_waitcnt vmcnt."""
    starts = [i for i, s in enumerate(ins) if s.startswith("buffer_load_dwordx2")]
    for i in starts:
        rsq = 0
        for s in ins[i + 1:] + ins[:i]:
            if s.startswith("v_rsq_f64"):
                rsq += 1
            elif s.startswith("s_waitcnt") and "vmcnt" in s:
                break
        if rsq < 2:
            return False
    return bool(starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--keep", default=None, help="write the assembly here")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = args.keep or os.path.join(tmp, "k.s")
        src = os.path.join(ROOT, "pyrayhf_amd", "csrc")
        subprocess.run([args.hipcc, *FLAGS, f"-I{ROOT}/include", f"-I{src}", "--offload-device-only", "-S",
                        os.path.join(src, "prhf_kernels.hip"), "-o", out], check=True)
        lines = open(out).read().splitlines()
    found = bad = 0
    start = None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w*lean_loop\w*):", l)
        if m:
            start, name = i, m.group(1)
        if start is not None and l.startswith("; ScratchSize:"):
            for label, ins in loops_of(lines[start:i]):
                text = "\n".join(ins)
                if all(k in text for k in ("ds_bpermute_b32", "global_load_dwordx4", "v_rsq_f64")) and \
                        text.count("v_rsq_f64") <= 4:                  # (the evaluation loop itself, not a loop around it)
                    ok = in_flight(ins)
                    found += 1
                    bad += not ok
                    print(f"{'ok  ' if ok else 'FAIL'} {name[:70]} {label}: {len(ins)} instructions")
            start = None
    print(f"{found} evaluation loops, {bad} with the look-up out of flight")
    return 1 if bad or not found else 0


if __name__ == "__main__":
    sys.exit(main())
