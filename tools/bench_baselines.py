#!/usr/bin/env python3
"""env-steps/s of the fused rollout for the Hungarian default and the two classical baselines (Local-PI, Local-Cap-Greedy) on the
same case and batch: WPS_hard_x2, 4096 envs, 150 steps, replan interval 20, observations written.  Same warm-up and timed-launch
protocol as bench.py (bench.time_rollouts: isolated warm-up launches, then `steps` launches queued back to back between two
synchronisations).  Each mode runs in a child process of its own under `timeout -k 10`.

    python tools/bench_baselines.py [--steps 20 --warmup 8 --envs 4096 --case WPS_hard_x2]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = ("hungarian", "pi", "cap_greedy")


def one(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    env = BatchedMultiUAVEnv(params_for_case(args.case), args.envs)
    env.set_allocator(args.one)
    seeds = np.arange(args.envs, dtype=np.uint64)
    elapsed, kernel_ms, _ = bench.time_rollouts(env, seeds, args.interval, True, args.steps, args.warmup, torch.cuda.synchronize)
    err = env.error_flags()
    ok = err == 0  # (an env that outgrows its tile stops with ERROR set: counted, and left out of the quality figures)
    m = env.rollout_metrics()[ok]
    print(json.dumps({"mode": args.one, "case": args.case, "envs": args.envs, "env_steps_per_s": args.envs * bench.HORIZON * args.steps / elapsed,
                      "mean_kernel_ms": kernel_ms, "capacity_flagged_envs": int((~ok).sum()),
                      "mean_S_WPS": float(m[:, 4].mean()),
                      "mean_n_replans": float(env.get("SCALARS")[:, 23].mean())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="WPS_hard_x2")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--interval", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--one", choices=MODES)
    args = ap.parse_args()
    if args.one:
        return one(args)
    rows = {}
    for mode in MODES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", mode, "--case", args.case,
               "--envs", str(args.envs), "--steps", str(args.steps), "--warmup", str(args.warmup), "--interval", str(args.interval)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # a fault or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"error": f"{mode}: exit status {r.returncode}", "done": rows}))
            sys.exit(1)
        rows[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[mode]), flush=True)
    h = rows["hungarian"]["env_steps_per_s"]
    print(json.dumps({"case": args.case, "envs": args.envs, **{f"{m}_env_steps_per_s": rows[m]["env_steps_per_s"] for m in MODES},
                      **{f"{m}_vs_hungarian": rows[m]["env_steps_per_s"] / h for m in ("pi", "cap_greedy")}}))


if __name__ == "__main__":
    main()
