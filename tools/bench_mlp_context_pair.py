#!/usr/bin/env python3
"""env-steps/s of the learned MLP-ContextPair policy (the sibling of tools/bench_mlp_pair.py): WPS_hard_x2 and WPS_attn, 4096 envs, 150
steps, replan interval 15, weight sets tests/golden/mlpctx_weights_init2.npz / mlppair_weights_init2.npz, per case from one session:

  torch_loop        the job done without the in-kernel forward pass: il.rl_run_stream with MLPContextPairNet's pair_mlp in torch on the
                    same GPU in the loop — pooled rows in torch, the context summary from muavta_context_device at every gate (one
                    launch more per gate than the MLP-Pair loop, and a sync before torch reads it)
  mlp_context_pair  the fused rollout with the MLP-ContextPair policy installed (the 192-wide network inside the kernel)
  mlp_pair          the fused rollout with the 128-wide MLP-Pair policy, same build
  urgency_pair      the fused rollout with the engineered score: the same planner without a network
  valid_share       the share of the 16 x 32 pairs whose edge_valid is 1 at the interval gates (the forward pass skips the others)

The fused modes use bench.py's protocol (bench.time_rollouts); the torch loop runs `warmup` whole batches, then `steps` timed ones.  Each
figure comes from a child process of its own under `timeout -k 10`; a failing child ends the run.

    python tools/bench_mlp_context_pair.py [--steps 10 --warmup 4 --envs 4096 --interval 15 --out profiles/mlp_context_pair_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = ("torch_loop", "mlp_context_pair", "mlp_pair", "urgency_pair", "valid_share")
CASES = ("WPS_hard_x2", "WPS_attn")


def load_weights(prefix, name):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{prefix}_weights_{name}.npz"))
    sd = {f"pair_mlp.{i}.{k}": np.ascontiguousarray(z[f"{n}{j}"], dtype=np.float32) for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}
    return sd, bool(z["raw_features"]), float(z["score_clamp"])


def one(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from muavta_amd import il
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    sd, raw, clamp = load_weights("mlpctx", args.weights)
    env = BatchedMultiUAVEnv(params_for_case(args.case), args.envs)
    seeds = np.arange(args.envs, dtype=np.uint64)
    kind = "pair_raw" if raw else "pair"
    row = {"mode": args.one, "case": args.case, "envs": args.envs, "interval": args.interval, "weights": args.weights}
    if args.one == "torch_loop":
        dev = torch.device("cuda", env.device_index)
        k0 = sd["pair_mlp.0.weight"].shape[1]
        mlp = torch.nn.Sequential(torch.nn.Linear(k0, 192), torch.nn.ReLU(), torch.nn.Linear(192, 192), torch.nn.ReLU(), torch.nn.Linear(192, 1)).to(dev)
        mlp.load_state_dict({k[len("pair_mlp."):]: torch.from_numpy(v) for k, v in sd.items()})
        mlp.eval()
        ctx = torch.empty((args.envs, 1 if raw else 8), dtype=torch.float32, device=dev)

        def policy(tok):  # MLPContextPairNet.forward (ContextPairHybrid.py:192-208) on the parked state's tokens
            env.context(kind, 32, out=ctx)
            env.sync()
            with torch.no_grad():
                af, tf = tok["agent_feats"], tok["task_feats"]
                am, tm = (tok["agent_mask"] == 0).float().unsqueeze(-1), (tok["task_mask"] == 0).float().unsqueeze(-1)
                a_pool, t_pool = (af * am).sum(1) / am.sum(1).clamp(min=1.0), (tf * tm).sum(1) / tm.sum(1).clamp(min=1.0)
                a, t = af.shape[1], tf.shape[1]
                uni = torch.cat([a_pool, t_pool, ctx], dim=-1).unsqueeze(1).unsqueeze(2).expand(-1, a, t, -1)
                pair = torch.cat([af.unsqueeze(2).expand(-1, -1, t, -1), tf.unsqueeze(1).expand(-1, a, -1, -1), uni], dim=-1)
                return (torch.tanh(mlp(pair).squeeze(-1)) * clamp * tok["edge_valid"]).contiguous()

        def batch():
            stepped = 0
            for _, tr in il.rl_run_stream(env, seeds, policy, interval=args.interval, kind=kind):
                stepped += int(tr["n_stepped"].sum().item())
            return stepped

        for _ in range(args.warmup):
            batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = sum(batch() for _ in range(args.steps))
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        row.update(env_steps_per_s=total / elapsed, env_steps=total, batches=args.steps, mean_S_WPS=float(env.metrics()[:, 4].mean()))
    elif args.one in ("mlp_context_pair", "mlp_pair", "urgency_pair"):
        if args.one == "mlp_context_pair":
            env.set_pair_policy(sd, clamp)
        elif args.one == "mlp_pair":
            sd128, _, clamp128 = load_weights("mlppair", args.weights)
            env.set_pair_policy(sd128, clamp128)
        env.set_allocator(args.one)
        res = bench.time_rollouts(env, seeds, args.interval, True, args.steps, args.warmup, torch.cuda.synchronize)
        ok = env.error_flags() == 0
        row.update(env_steps_per_s=args.envs * bench.HORIZON * args.steps / res[0], mean_kernel_ms=res[1], capacity_flagged_envs=int((~ok).sum()),
                   mean_S_WPS=float(env.rollout_metrics()[ok][:, 4].mean()), mean_n_replans=float(env.get("SCALARS")[:, 23].mean()))
    else:
        n = min(args.envs, 512)
        small = BatchedMultiUAVEnv(params_for_case(args.case), n)
        small.set_pair_policy(sd, clamp)
        small.set_allocator("mlp_context_pair")
        small.reset(np.arange(n, dtype=np.uint64))
        shares = []
        for t in range(bench.HORIZON):
            if t % args.interval == 0:
                shares.append(float(small.tokens(kind, 32, 16)["edge_valid"].mean()))
            small.allocate(args.interval, True, fetch=False)
            small.step_staged()
        row.update(valid_share=float(np.mean(shares)), valid_share_min=float(np.min(shares)), valid_share_max=float(np.max(shares)), envs=n)
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="one case (default: WPS_hard_x2 and WPS_attn)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--interval", type=int, default=15)
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
        fused = rows["mlp_context_pair"]["env_steps_per_s"]
        out["cases"][case] = {**{f"{m}_env_steps_per_s": rows[m]["env_steps_per_s"] for m in MODES[:4]}, "valid_share": rows["valid_share"]["valid_share"],
                              "mlp_context_pair_vs_torch_loop": fused / rows["torch_loop"]["env_steps_per_s"],
                              "mlp_context_pair_vs_mlp_pair": fused / rows["mlp_pair"]["env_steps_per_s"],
                              "mlp_context_pair_vs_urgency_pair": fused / rows["urgency_pair"]["env_steps_per_s"], "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
