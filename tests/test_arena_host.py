"""Host check of the scratch-buffer carver (pyrayhf_amd/csrc/prhf_arena.h), no GPU: tests/devtools/arena_host.cpp,
a stand-alone program, built plain and under ASan + UBSan.  A buffer's layout is stated once and run twice - over a null
base for its size, over the buffer for its pointers - so the program pins that the two passes agree and that the mixed
layout of the gradient tracers' MUF scratch lands where the hand-written arithmetic before it put it.  It includes
prhf_layouts.h, the arena's blocks of the operator, the residual stages and the stage ops as the library compiles them:
for each, the size and every offset against the hand arithmetic they replaced, and a write to the block's last element
inside a buffer of exactly used() bytes."""

import os
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("sanitize", [False, True])
def test_carver(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    exe = tmp_path / "arena_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", *extra, "-I", os.path.join(REPO, "pyrayhf_amd", "csrc"),
                    os.path.join(REPO, "tests", "devtools", "arena_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "arena_host: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
