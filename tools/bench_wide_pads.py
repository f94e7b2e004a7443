#!/usr/bin/env python3
"""env-steps/s of the pair-cost planners at the wide token pads (set_token_pads(64, 48)) on the reference's scale cases (WPS_attn_L,
WPS_attn_XL; 4096 envs, 150 steps, replan interval 15, weight sets init2 of tests/golden), per case from one session:

  urgency_pair            the fused rollout with the engineered score over the 48 x 64 grid
  mlp_pair                the fused rollout in the MUAVTA_ALLOC_MLP_PAIR mode with an MLP-Pair, the network inside the kernel
  mlp_context_pair        the same with an MLP-ContextPair
  torch_pair / torch_ctx  the job done without the in-kernel forward pass: il.rl_run_stream at max_tasks = 64, max_agents = 48 with a torch
                          MLP that holds the same weights on the same GPU in the loop (one launch, one sync and one torch forward per gate)
  valid_share             the share of the 48 x 64 pairs whose edge_valid is 1 at the interval gates (the forward pass skips the others)

The protocol is tools/bench_mlp_pair.py's: bench.time_rollouts for the fused modes, whole batches for the torch loops, each figure from a
child process of its own under `timeout -k 10`; a failing child ends the run.  There is no target figure: these rows have never run.

    python tools/bench_wide_pads.py [--steps 6 --warmup 2 --envs 4096 --interval 15 --out profiles/wide_pads_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
MODES = ("urgency_pair", "mlp_pair", "mlp_context_pair", "torch_pair", "torch_ctx", "valid_share")
CASES = ("WPS_attn_L", "WPS_attn_XL")
MT, MA = 64, 48

from bench_mlp_context_pair import load_weights  # noqa: E402


def one(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from muavta_amd import il
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    ctx_kind = args.one in ("mlp_context_pair", "torch_ctx")
    sd, raw, clamp = load_weights("mlpctx" if ctx_kind else "mlppair", args.weights)
    n = min(args.envs, 512) if args.one == "valid_share" else args.envs
    env = BatchedMultiUAVEnv(params_for_case(args.case), n)
    env.set_token_pads(MT, MA)
    seeds = np.arange(n, dtype=np.uint64)
    kind = "pair_raw" if raw else "pair"
    row = {"mode": args.one, "case": args.case, "envs": n, "interval": args.interval, "weights": args.weights, "token_pads": [MT, MA]}
    if args.one in ("torch_pair", "torch_ctx"):
        dev = torch.device("cuda", env.device_index)
        k0, hid = sd["pair_mlp.0.weight"].shape[1], sd["pair_mlp.0.weight"].shape[0]
        mlp = torch.nn.Sequential(torch.nn.Linear(k0, hid), torch.nn.ReLU(), torch.nn.Linear(hid, hid), torch.nn.ReLU(), torch.nn.Linear(hid, 1)).to(dev)
        mlp.load_state_dict({k[len("pair_mlp."):]: torch.from_numpy(v) for k, v in sd.items()})
        mlp.eval()
        ctx = torch.empty((n, 1 if raw else 8), dtype=torch.float32, device=dev)

        def policy(tok):  # PairCostHybrid.act / MLPContextPairNet.forward (ContextPairHybrid.py:192-208) on the parked state's tokens
            if ctx_kind:
                env.context(kind, MT, out=ctx)
                env.sync()
            with torch.no_grad():
                af, tf = tok["agent_feats"], tok["task_feats"]
                a, t = af.shape[1], tf.shape[1]
                cols = [af.unsqueeze(2).expand(-1, -1, t, -1), tf.unsqueeze(1).expand(-1, a, -1, -1)]
                if ctx_kind:
                    am, tm = (tok["agent_mask"] == 0).float().unsqueeze(-1), (tok["task_mask"] == 0).float().unsqueeze(-1)
                    a_pool, t_pool = (af * am).sum(1) / am.sum(1).clamp(min=1.0), (tf * tm).sum(1) / tm.sum(1).clamp(min=1.0)
                    cols.append(torch.cat([a_pool, t_pool, ctx], dim=-1).unsqueeze(1).unsqueeze(2).expand(-1, a, t, -1))
                return (torch.tanh(mlp(torch.cat(cols, dim=-1)).squeeze(-1)) * clamp * tok["edge_valid"]).contiguous()

        def batch():
            stepped = 0
            for _, tr in il.rl_run_stream(env, seeds, policy, interval=args.interval, kind=kind, max_tasks=MT, max_agents=MA):
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
    elif args.one == "valid_share":
        env.set_allocator("urgency_pair")
        env.reset(seeds)
        shares = []
        for t in range(bench.HORIZON):
            if t % args.interval == 0:
                shares.append(float(env.tokens(kind, MT, MA)["edge_valid"].mean()))
            env.allocate(args.interval, True, fetch=False)
            env.step_staged()
        row.update(valid_share=float(np.mean(shares)), valid_share_min=float(np.min(shares)), valid_share_max=float(np.max(shares)))
    else:
        if args.one != "urgency_pair":
            env.set_pair_policy(sd, clamp)
        env.set_allocator(args.one)
        res = bench.time_rollouts(env, seeds, args.interval, True, args.steps, args.warmup, torch.cuda.synchronize)
        ok = env.error_flags() == 0
        row.update(env_steps_per_s=n * bench.HORIZON * args.steps / res[0], mean_kernel_ms=res[1], capacity_flagged_envs=int((~ok).sum()),
                   mean_S_WPS=float(env.rollout_metrics()[ok][:, 4].mean()), mean_n_replans=float(env.get("SCALARS")[:, 23].mean()))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--interval", type=int, default=15)
    ap.add_argument("--weights", default="init2")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=MODES)
    args = ap.parse_args()
    if args.one:
        return one(args)
    out = {"envs": args.envs, "interval": args.interval, "weights": args.weights, "token_pads": [MT, MA], "cases": {}}
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
        out["cases"][case] = {**{f"{m}_env_steps_per_s": rows[m]["env_steps_per_s"] for m in MODES[:5]}, "valid_share": rows["valid_share"]["valid_share"],
                              "mlp_pair_vs_torch_pair": rows["mlp_pair"]["env_steps_per_s"] / rows["torch_pair"]["env_steps_per_s"],
                              "mlp_context_pair_vs_torch_ctx": rows["mlp_context_pair"]["env_steps_per_s"] / rows["torch_ctx"]["env_steps_per_s"], "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
