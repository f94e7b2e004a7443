#!/usr/bin/env python3
"""env-steps/s of the learned MLP-Coalition policy (the sibling of tools/bench_mlp_context_pair.py): WPS_escort and WPS_escort24, 4096
envs, 150 steps, replan interval 12, weight set tests/golden/mlpcoal_weights_init2.npz, per case from one session:

  torch_loop         the job done without the in-kernel forward pass: il.rl_run_stream (escort tokens 16 x 48, gate `escort`, commit locks)
                     with MLPCoalitionNet's pair_mlp in torch on the same GPU in the loop — the yardstick
  mlp_coalition      the fused rollout with the MLP-Coalition policy installed (the 256-wide network inside the kernel)
  urgency_coalition  the fused rollout with the engineered score: the same planner without a network — the ceiling
  valid_share        the share of the 16 x 48 pairs whose edge_valid is 1 at the plans of the mode (the forward pass skips the others)

The fused modes use bench.py's protocol (bench.time_rollouts); the torch loop runs `warmup` whole batches, then `steps` timed ones.  Each
figure comes from a child process of its own under `timeout -k 10`; a failing child ends the run.

    python tools/bench_mlp_coalition.py [--steps 10 --warmup 4 --envs 4096 --interval 12 --out profiles/mlp_coalition_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = ("torch_loop", "mlp_coalition", "urgency_coalition", "valid_share")
CASES = ("WPS_escort", "WPS_escort24")


def load_weights(name):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"mlpcoal_weights_{name}.npz"))
    return {f"pair_mlp.{i}.{k}": np.ascontiguousarray(z[f"{n}{j}"], dtype=np.float32) for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}


def one(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from muavta_amd import il
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    sd = load_weights(args.weights)
    env = BatchedMultiUAVEnv(params_for_case(args.case), args.envs)
    seeds = np.arange(args.envs, dtype=np.uint64)
    row = {"mode": args.one, "case": args.case, "envs": args.envs, "interval": args.interval, "weights": args.weights}
    if args.one == "torch_loop":
        dev = torch.device("cuda", env.device_index)
        mlp = torch.nn.Sequential(torch.nn.Linear(38, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 1)).to(dev)
        mlp.load_state_dict({k[len("pair_mlp."):]: torch.from_numpy(v) for k, v in sd.items()})
        mlp.eval()

        def policy(tok):  # MLPCoalitionNet.forward + AttentionEscort.act (AttentionEscort.py:356-364,465-469) on the parked state's tokens
            with torch.no_grad():
                af, tf = tok["agent_feats"], tok["task_feats"]
                a, t = af.shape[1], tf.shape[1]
                pair = torch.cat([af.unsqueeze(2).expand(-1, -1, t, -1), tf.unsqueeze(1).expand(-1, a, -1, -1)], dim=-1)
                live = (tok["agent_mask"] == 0).float().unsqueeze(2) * (tok["task_mask"] == 0).float().unsqueeze(1)
                return (torch.sigmoid(mlp(pair).squeeze(-1).clamp(-20, 20)) * tok["edge_valid"] * live).contiguous()

        def batch():
            stepped = 0
            for _, tr in il.rl_run_stream(env, seeds, policy, interval=args.interval, kind="escort", max_tasks=48, max_agents=16, gate="escort",
                                          edge_valid_only=False, commit=True):
                stepped += int(tr["n_stepped"].sum().item())
            return stepped

        for _ in range(args.warmup):
            batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = sum(batch() for _ in range(args.steps))
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        import muavta_amd.batched as batched
        m = np.empty((args.envs, batched.N_METRICS), dtype=np.float64)  # (env.metrics() raises where an env outgrew its tile; the rows are filled all the same)
        rc = env.L.muavta_metrics(env.h, m.ctypes.data)
        if rc not in (0, -4):
            raise RuntimeError(env.L.muavta_last_error(env.h).decode())
        ok = ~env.get("ERROR").reshape(args.envs, -1).any(axis=1)
        row.update(env_steps_per_s=total / elapsed, env_steps=total, batches=args.steps, capacity_flagged_envs=int((~ok).sum()), mean_S_ESC=float(m[ok][:, 5].mean()))
    elif args.one in ("mlp_coalition", "urgency_coalition"):
        if args.one == "mlp_coalition":
            env.set_pair_policy(sd)
        env.set_allocator(args.one)
        res = bench.time_rollouts(env, seeds, args.interval, True, args.steps, args.warmup, torch.cuda.synchronize)
        ok = env.error_flags() == 0
        row.update(env_steps_per_s=args.envs * bench.HORIZON * args.steps / res[0], mean_kernel_ms=res[1], capacity_flagged_envs=int((~ok).sum()),
                   mean_S_ESC=float(env.rollout_metrics()[ok][:, 5].mean()), mean_n_replans=float(env.get("SCALARS")[:, 23].mean()))
    else:
        n = min(args.envs, 512)
        small = BatchedMultiUAVEnv(params_for_case(args.case), n)
        small.set_pair_policy(sd)
        small.set_allocator("mlp_coalition")
        small.reset(np.arange(n, dtype=np.uint64))
        shares, last = [], np.zeros(n, dtype=np.int64)
        for t in range(bench.HORIZON):
            ev = small.tokens("escort", 48, 16)["edge_valid"].mean(axis=(1, 2))
            small.allocate(args.interval, True, fetch=False)
            reps = small.get("SCALARS")[:, 23].astype(np.int64)
            shares.extend(ev[reps > last].tolist())   # the envs that planned at this step
            last = reps
            small.step_staged()
        row.update(valid_share=float(np.mean(shares)), valid_share_max=float(np.max(shares)), plans=len(shares), mean_n_replans=float(last.mean()), envs=n)
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="one case (default: WPS_escort and WPS_escort24)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--interval", type=int, default=12)
    ap.add_argument("--weights", default="init2")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=MODES)
    args = ap.parse_args()
    if args.one:
        return one(args)
    out = {"envs": args.envs, "interval": args.interval, "weights": args.weights, "cases": {}}
    for case in ([args.case] if args.case else CASES):
        rows = {}
        for mode in MODES:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", mode, "--case", case, "--envs", str(args.envs),
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--interval", str(args.interval), "--weights", args.weights]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # a fault or a time limit: nothing more is started on the GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(json.dumps({"error": f"{case} {mode}: exit status {r.returncode}", "done": out}))
                sys.exit(1)
            rows[mode] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rows[mode]), flush=True)
        fused = rows["mlp_coalition"]["env_steps_per_s"]
        out["cases"][case] = {**{f"{m}_env_steps_per_s": rows[m]["env_steps_per_s"] for m in MODES[:3]}, "valid_share": rows["valid_share"]["valid_share"],
                              "mean_n_replans": rows["mlp_coalition"]["mean_n_replans"], "mlp_coalition_kernel_ms": rows["mlp_coalition"]["mean_kernel_ms"],
                              "urgency_coalition_kernel_ms": rows["urgency_coalition"]["mean_kernel_ms"],
                              "mlp_coalition_vs_torch_loop": fused / rows["torch_loop"]["env_steps_per_s"],
                              "mlp_coalition_vs_urgency_coalition": fused / rows["urgency_coalition"]["env_steps_per_s"], "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
