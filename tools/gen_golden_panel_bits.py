#!/usr/bin/env python
"""Write tests/golden/g27_panel_bits.npz: the virtual heights, to the bit, and the panel sum's counters of the launches
of tests/panel_bits_cases.py, with the `hipcc --version` line of the build.  Outputs only: the inputs come from the
helpers' seeds.  Needs a GPU.

Run it on the commit whose bits are to be kept - it uses nothing but _native.Context's public calls, so it runs on any
commit that has the options panel_nodes and panel_upper - before a change of the panel block of lean_loop_body that
must not move a bit; tests/test_gpu_panel_pipeline.py then compares the changed build with it.

Usage: python tools/gen_golden_panel_bits.py [output file]
"""

from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import panel_bits_cases as cases                         # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g27_panel_bits.npz")


def main(out):
    ctxs = {nodes: cases.make_context(panel_nodes=nodes) for nodes in (4, 8)}
    data = {"hipcc": np.array(cases.hipcc_version_line())}
    for name, (nodes, args, kwargs) in cases.inputs().items():
        vh, counted = cases.launch(ctxs[nodes], *args, **kwargs)
        again, counted2 = cases.launch(ctxs[nodes], *args, **kwargs)
        assert vh.tobytes() == again.tobytes() and np.array_equal(counted, counted2), name
        assert not (vh == -7.0).any(), name
        data[f"{name}_vh"] = vh
        data[f"{name}_counters"] = counted
        print(f"{name}: {vh.shape}, {int(np.isfinite(vh).sum())} finite; took {counted[0]}, fell back {counted[1]}, "
              f"reached the top segment {counted[2]}, kept the lower region {counted[3]}")
    for c in ctxs.values():
        c.close()
    np.savez_compressed(out, **data)
    print(f"{out}: {os.path.getsize(out)} bytes; {data['hipcc']}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
