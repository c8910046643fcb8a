"""Per-wave timeline of the fused kernel (needs a -DPRHF_TRACE build of libprhf.so, PRHF_LIB pointing at it) on the
config-4 shard.  Prints how full the wave slots of a workgroup are over its life, how the launch drains, and the account
of the serial work around the sum: staging by phase, the wait at the end-of-block barrier, the queue's turnaround - or,
for the streaming form (option stream_blocks), the time a wave polls for a ready slot and the stager's time by phase.
Context options: PRHF_TOOL_OPTIONS="name=value,..." (tools/_options.py); PRHF_TRACE_FORM=stream reads the records of the
streaming form.

A record is eight words per wave and block.  General kernel: start, arrival at the end-of-block barrier, candidate list
made (every wave its own), then thread 0's marks - argmax known, nodes staged, running maximum done, pairs planned -
and the workgroup.  Streaming form: arrival at the slot, leaving it, slot seen ready, then the stager's marks (the same
four behind its own start in word 7; zero in the records of the other waves) - sixteen waves per block."""
import os, sys, json
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
import _options
path = os.environ.get("PRHF_TRACE_OUT", "/tmp/prhf_trace.bin")
os.environ["PRHF_TRACE_FILE"] = path
from pyrayhf_amd import library, synth
options = _options.apply()
dev = torch.device("cuda", 0)
alt, den, bmag, bpsi = synth.chapman_profiles(12500, 20260004)
t = [torch.as_tensor(x, device=dev) for x in (synth.sounder_frequencies(4), den, bmag, bpsi, alt)]
for _ in range(2):
    library.vertical_forward_operator(*t, "X", 20000)
raw = np.fromfile(path, dtype=np.uint64)
W = 16 if os.environ.get("PRHF_TRACE_FORM", "") == "stream" else 8     # (the streaming form's launches: sixteen waves per block)
raw = raw.reshape(-1, W, 8)
raw = raw[raw[:, :, 1].max(axis=1) > 0]
w = raw.astype(np.float64) / 100.0  # us (100 MHz wall clock)
t0 = w[:, :, 0].min()
start, end = w[:, :, 0] - t0, w[:, :, 1] - t0
wg_start, wg_end = start.min(axis=1), end.max(axis=1)
life = wg_end - wg_start
fill = (end - start).sum(axis=1) / (W * life)
print(json.dumps({"options": options, "waves_per_block": W, "workgroups": int(w.shape[0]), "kernel_us": float(wg_end.max()),
                  "wg_life_us": {"mean": float(life.mean()), "p10": float(np.percentile(life, 10)), "p90": float(np.percentile(life, 90)), "max": float(life.max())},
                  "wave_slot_fill_within_wg": {"mean": float(fill.mean()), "p10": float(np.percentile(fill, 10)), "weighted": float(((end - start).sum()) / (W * life.sum()))},
                  "first_wave_done_frac_of_life": float(((end.min(axis=1) - wg_start) / life).mean()),
                  "median_wave_done_frac_of_life": float(((np.median(end, axis=1) - wg_start) / life).mean())}))


def stats(x):
    return "mean %.2f  p50 %.2f  p90 %.2f  max %.2f" % (x.mean(), np.percentile(x, 50), np.percentile(x, 90), x.max())


if W == 8:
    # ---- the general kernel: all eight waves go through staging barrier to barrier, then wait for the slowest one ----
    m = w[:, :, 3:7].max(axis=1) - t0          # thread 0's marks (every wave copied them)
    listed = w[:, 0, 2] - t0                   # wave 0 has the candidate list
    listed_all = w[:, :, 2].max(axis=1) - t0   # ... the last wave has it
    phases = {"argmax (phase 1, first barrier)": m[:, 0] - wg_start, "nodes (phase 2, second barrier)": m[:, 1] - m[:, 0],
              "running maximum (O mode only)": m[:, 2] - m[:, 1], "list_candidates (wave 0)": listed - m[:, 2],
              "plan_pairs": m[:, 3] - listed}
    print("staging per block [us], by phase:")
    for name, x in phases.items():
        print("  %-34s %s" % (name, stats(x)))
    staging = m[:, 3] - wg_start
    print("  %-34s %s" % ("all of staging", stats(staging)))
    print("  %-34s %s" % ("list made, last wave - wave 0", stats(listed_all - listed)))
    wait = wg_end[:, None] - end
    print("wait per wave at the end-of-block barrier [us]:", stats(wait.mean(axis=1)), " (per block: mean over its waves)")
    # the queue's turnaround: a workgroup's blocks in order of start
    wg = raw[:, 0, 7].astype(np.int64)
    order = np.lexsort((wg_start, wg))
    same = wg[order][1:] == wg[order][:-1]
    turn = (wg_start[order][1:] - wg_end[order][:-1])[same]
    print("queue turnaround between two blocks of a workgroup [us]:", stats(turn))
    wave_time = W * (life.sum() + turn.sum())
    parts = {"staging": W * staging.sum(), "barrier wait": wait.sum(), "queue turnaround": W * turn.sum()}
    print("share of wave-time:", {k: round(float(v / wave_time), 4) for k, v in parts.items()},
          "together %.4f" % (sum(parts.values()) / wave_time))
    # the waves that compute during list_candidates (256 of 512 threads) and plan_pairs (~130) are counted as held:
    # the ceiling is what an overlap could give back at most
    print("staging time per workgroup [us] (start to list made, as before): mean %.2f  p90 %.2f"
          % ((w[:, :, 2] - w[:, :, 0]).max(axis=1).mean(), np.percentile((w[:, :, 2] - w[:, :, 0]).max(axis=1), 90)))
else:
    # ---- the streaming form: a wave polls until the slot is ready; one wave staged it beside the others ----
    ready = w[:, :, 2] - t0
    poll = ready - start
    print("poll for a ready slot per wave and block [us]:", stats(poll.reshape(-1)))
    is_stager = w[:, :, 7] > 0
    sm = w[:, :, 3:8] - t0
    s_begin = sm[:, :, 4][is_stager]
    marks = [sm[:, :, i][is_stager] for i in range(4)]
    names = ["argmax (phase 1)", "nodes (phase 2)", "list_candidates", "plan_pairs and publish"]
    prev = s_begin
    print("stager per block [us], by phase:")
    for name, x in zip(names, marks):
        print("  %-34s %s" % (name, stats(x - prev)))
        prev = x
    staging = marks[3] - s_begin
    print("  %-34s %s" % ("all of staging", stats(staging)))
    # a wave's time: from its first arrival to its last leave; blocks of the launch are visited by every wave of the workgroup
    wave_time = (end - start).sum()
    print("share of wave-time:", {"polling": round(float(poll.sum() / wave_time), 4),
                                  "stager": round(float(staging.sum() / wave_time), 4)})
print("mean finish time of wave w as a fraction of its workgroup's life:",
      [round(float(x), 3) for x in ((end - wg_start[:, None]) / life[:, None]).mean(axis=0)])
print("mean start delay of wave w [us]:", [round(float(x), 2) for x in (start - wg_start[:, None]).mean(axis=0)])
# resident workgroups over time
edges = np.linspace(0, wg_end.max(), 41)
res = [(np.minimum(wg_end, b) - np.maximum(wg_start, a)).clip(0).sum() / (b - a) for a, b in zip(edges[:-1], edges[1:])]
print("resident blocks per 1/40 of the launch:", [round(x) for x in res])
waves = [(np.minimum(end, b) - np.maximum(start, a)).clip(0).sum() / (b - a) for a, b in zip(edges[:-1], edges[1:])]
print("resident waves per 1/40 of the launch:", [round(x) for x in waves])
