"""bench.py on the GPU: a plain run prints the headline line and nothing of what --full adds, and --dump-outputs
writes what the timed steps computed, as finite arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_steps_virtual_heights(tmp_path):
    import torch

    from pyrayhf_amd import library, synth
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--profiles", "600", "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-3000:]
    line = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["unit"] == "integrals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["ms_per_step"] > 0.0 and line["value"] > 0.0
    assert abs(line["value"] - 600 * 256 / (1e-3 * line["ms_per_step"])) <= 1e-6 * line["value"]
    moved = {"cpu_baseline", "cpu_baseline_all_cores", "single_profile", "dropin_call", "host_buffers", "config3",
             "config5_shard", "config4_full", "snell_per_ray", "stage_ops", "fit_brute", "devices_all"}
    assert not moved & set(line), sorted(moved & set(line))

    vh, reflects = np.load(tmp_path / "out" / "vh.npy"), np.load(tmp_path / "out" / "reflects.npy")
    assert vh.dtype == reflects.dtype == np.float64 and vh.shape == reflects.shape == (600, 256)
    assert np.isfinite(vh).all() and np.isin(reflects, (0.0, 1.0)).all()
    # the bench's rows of config 4's draw through the library in this process
    alt, den, bmag, bpsi = synth.chapman_profiles(100000, 20260004, rows=slice(0, 600))
    dev = torch.device("cuda", 0)
    want = library.vertical_forward_operator(*[torch.as_tensor(x, device=dev) for x in
                                               (np.linspace(0.5, 16.0, 256), den, bmag, bpsi, alt)], "X", 20000)
    want = want.cpu().numpy()
    assert 0.0 < reflects.mean() < 1.0 and np.array_equal(reflects, np.isfinite(want))
    np.testing.assert_allclose(vh, np.nan_to_num(want, nan=0.0), rtol=1e-12, atol=0.0)
