#!/usr/bin/env python3
"""Summary of a rocprofv3 --kernel-trace CSV of bench.py: which hardware queue every k_seed / k_rollout dispatch of the queued
launches ran on, and whether consecutive rollouts overlapped.  usage: queue_trace_summary.py <dir or *_kernel_trace.csv> [last_n]"""
import collections
import csv
import glob
import os
import sys


def main():
    path = sys.argv[1]
    last_n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*_kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit(f"no *_kernel_trace.csv under {path}")
        path = found[0]
    rows = list(csv.DictReader(open(path)))
    print("trace", os.path.basename(path), "dispatches", len(rows))
    roll = sorted((r for r in rows if "k_rollout" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    seed = sorted((r for r in rows if "k_seed" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    if len(roll) < 2:
        raise SystemExit("fewer than two k_rollout dispatches")
    # the largest grid is the benchmark's batch; its last `last_n` dispatches are the launches queued back to back
    gkey = "Grid_Size_X" if "Grid_Size_X" in roll[0] else "Grid_Size"
    grid = max(int(r[gkey]) for r in roll)
    sel = [r for r in roll if int(r[gkey]) == grid][-last_n:]
    t0, t1 = int(sel[0]["Start_Timestamp"]), int(sel[-1]["End_Timestamp"])
    sd = [r for r in seed if t0 - 5_000_000 <= int(r["Start_Timestamp"]) <= t1]
    q_roll = collections.Counter(r["Queue_Id"] for r in sel)
    q_seed = collections.Counter(r["Queue_Id"] for r in sd)
    if "Stream_Id" in sel[0]:  # which HIP streams each hardware queue carried, over the whole run
        streams = collections.defaultdict(set)
        for r in rows:
            streams[r["Queue_Id"]].add(r["Stream_Id"])
        print("streams per queue (whole run):", {q: sorted(v, key=int) for q, v in sorted(streams.items())})
        print("k_rollout streams:", dict(collections.Counter(r["Stream_Id"] for r in sel)), "k_seed streams:", dict(collections.Counter(r["Stream_Id"] for r in sd)))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in sel]
    gaps = [(int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) / 1e6 for a, b in zip(sel, sel[1:])]
    print(f"k_rollout: last {len(sel)} dispatches of grid {grid}: queues {dict(q_roll)}")
    print(f"  mean duration {sum(dur) / len(dur):.3f} ms, span per launch {(t1 - t0) / 1e6 / len(sel):.3f} ms")
    print(f"  start(i+1) - end(i): mean {sum(gaps) / len(gaps):.3f} ms, min {min(gaps):.3f}, max {max(gaps):.3f}; overlapping successors {sum(g < 0 for g in gaps)} of {len(gaps)}")
    print(f"k_seed: {len(sd)} dispatches in the same window: queues {dict(q_seed)}")
    shared = set(q_roll) & set(q_seed)
    print("  queues that carried both k_seed and k_rollout:", sorted(shared) if shared else "none")
    # a k_seed that STARTS while a rollout on ANOTHER queue runs ran beside it; one that starts at a rollout's end waited for it
    beside = 0
    for s in sd:
        ss = int(s["Start_Timestamp"])
        beside += any(int(r["Start_Timestamp"]) < ss < int(r["End_Timestamp"]) for r in sel)
    print(f"  k_seed dispatches that started while a k_rollout was running: {beside} of {len(sd)}")
    print("  timeline (ms from the first; kernel, queue, start, end):")
    ev = sorted(sel + sd, key=lambda r: int(r["Start_Timestamp"]))[-24:]
    for r in ev:
        name = "k_seed   " if "k_seed" in r["Kernel_Name"] else "k_rollout"
        print(f"    {name} q{r['Queue_Id']:>3} {(int(r['Start_Timestamp']) - t0) / 1e6:9.3f} {(int(r['End_Timestamp']) - t0) / 1e6:9.3f}")


if __name__ == "__main__":
    main()
