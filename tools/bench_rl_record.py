#!/usr/bin/env python3
"""What recording the RL transitions inside the fused rollout costs, and what it replaces: env-steps/s of one case and batch (WPS_hard_x2,
4096 envs, 150 steps, replan interval 20, weight sets tests/golden/mlp{pair,ctx}_weights_init2.npz), for MLP-Pair and MLP-ContextPair, all
rows of a policy from ONE process, alternating, each with its own warm-up:

  a  rollout          the plain fused rollout in 'mlp_pair' mode — measured three times (before b, before c, before d): the spread of the
                      three is the run-to-run spread every ratio below is read against
  b  rl_record        `rollout_rl_record` without noise, 64 slots
  c  rl_record_noise  the same with exploration noise: `torch.randn * 0.2` into the noise ring on the same GPU before every launch
  d  torch_loop       `il.rl_run_stream` with the same network as a torch module in the loop: one launch, one sync and one torch forward per gate

a, b and c queue `steps` launches back to back between two synchronisations (bench.py's protocol; b and c alternate between two ring sets,
as the two state lanes alternate); d runs whole batches one after another.  Also reported: valid transitions per second, the share of envs
with more than 64 gates, the bytes of one ring set.

    python tools/bench_rl_record.py [--steps 6 --warmup 3 --envs 4096 --case WPS_hard_x2 --interval 20 --slots 64 --out profiles/rl_record_bench.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HORIZON = 150


def load_weights(prefix, name):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{prefix}_weights_{name}.npz"))
    sd = {f"pair_mlp.{i}.{k}": np.ascontiguousarray(z[f"{n}{j}"], dtype=np.float32) for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}
    return sd, bool(z["raw_features"]), float(z["score_clamp"])


def torch_policy(kind, sd, clamp, dev):
    """the network of `sd` as a torch module: tok -> scores [N, 16, 32] (MLP-ContextPair: with the pooled rows and a zero context — the
    forward pass costs the same whatever the context holds, and row d is a timing)"""
    import torch
    k0, hid = sd["pair_mlp.0.weight"].shape[1], sd["pair_mlp.0.weight"].shape[0]
    mlp = torch.nn.Sequential(torch.nn.Linear(k0, hid), torch.nn.ReLU(), torch.nn.Linear(hid, hid), torch.nn.ReLU(), torch.nn.Linear(hid, 1)).to(dev)
    mlp.load_state_dict({k[len("pair_mlp."):]: torch.from_numpy(v) for k, v in sd.items()})
    mlp.eval()

    def policy(tok):
        with torch.no_grad():
            af, tf = tok["agent_feats"], tok["task_feats"]
            cols = [af.unsqueeze(2).expand(-1, -1, tf.shape[1], -1), tf.unsqueeze(1).expand(-1, af.shape[1], -1, -1)]
            if kind == "context":
                am, tm = (tok["agent_mask"] == 0).float().unsqueeze(-1), (tok["task_mask"] == 0).float().unsqueeze(-1)
                a_pool = (af * am).sum(1) / am.sum(1).clamp(min=1)
                t_pool = (tf * tm).sum(1) / tm.sum(1).clamp(min=1)
                env_in = torch.cat([a_pool, t_pool, torch.zeros((af.shape[0], k0 - 2 * (af.shape[2] + tf.shape[2])), device=dev)], dim=1)
                cols.append(env_in[:, None, None, :].expand(-1, af.shape[1], tf.shape[1], -1))
            return (torch.tanh(mlp(torch.cat(cols, dim=-1)).squeeze(-1)) * clamp * tok["edge_valid"]).contiguous()
    return policy


def measure(kind, args):
    import numpy as np
    import torch

    from muavta_amd import il
    from muavta_amd.batched import BatchedMultiUAVEnv
    from muavta_amd.params import params_for_case

    sd, raw, clamp = load_weights("mlpctx" if kind == "context" else "mlppair", args.weights)
    env = BatchedMultiUAVEnv(params_for_case(args.case), args.envs)
    env.set_pair_policy(sd, clamp)
    env.set_allocator("mlp_pair")
    dev = torch.device("cuda", env.device_index)
    seeds = np.arange(args.envs, dtype=np.uint64)
    G, N = args.slots, args.envs
    tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
    sets = [{name: torch.empty(shape, dtype=tdt[dtype], device=dev) for name, (shape, dtype) in env.rl_record_shapes(G).items()} for _ in range(2)]
    # (one noise ring per queued launch: torch's stream fills ring i while earlier launches may still be running on the handle's)
    noises = [torch.empty((G, N, 16, 32), dtype=torch.float32, device=dev) for _ in range(max(args.steps, args.warmup))]
    ring_bytes = sum(t.numel() * t.element_size() for t in sets[0].values())
    steps_per_launch = N * HORIZON

    def timed(launch, steps=args.steps):
        for i in range(args.warmup):
            launch(i)
        env.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            launch(i)
        env.sync(); torch.cuda.synchronize()
        return time.perf_counter() - t0

    def plain(i):
        env.rollout(seeds, HORIZON, args.interval, True, True)

    def rec(i):
        env.rollout_rl_record(seeds, HORIZON, args.interval, True, sets[i & 1], write_obs=True)

    def rec_noise(i):
        torch.randn(noises[i].shape, dtype=torch.float32, device=dev, out=noises[i]).mul_(0.2)
        env.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
        env.rollout_rl_record(seeds, HORIZON, args.interval, True, sets[i & 1], noise=noises[i], write_obs=True)

    rows, a = {}, []
    a.append(steps_per_launch * args.steps / timed(plain))
    t = timed(rec)
    ng = sets[(args.steps - 1) & 1]["n_gates"].cpu().numpy()
    rows["rl_record"] = {"env_steps_per_s": steps_per_launch * args.steps / t, "valid_transitions_per_s": float(np.minimum(ng, G).sum()) * args.steps / t,
                         "mean_gates_per_env": float(ng.mean()), "share_envs_over_slots": float((ng > G).mean())}
    a.append(steps_per_launch * args.steps / timed(plain))
    t = timed(rec_noise)
    ng = sets[(args.steps - 1) & 1]["n_gates"].cpu().numpy()
    rows["rl_record_noise"] = {"env_steps_per_s": steps_per_launch * args.steps / t, "valid_transitions_per_s": float(np.minimum(ng, G).sum()) * args.steps / t,
                               "mean_gates_per_env": float(ng.mean()), "share_envs_over_slots": float((ng > G).mean())}
    a.append(steps_per_launch * args.steps / timed(plain))
    flagged = int((env.error_flags() != 0).sum())
    policy = torch_policy(kind, sd, clamp, dev)
    stepped = [0]

    def loop(i):
        for _, tr in il.rl_run_stream(env, seeds, policy, interval=args.interval, kind="pair_raw" if raw else "pair"):
            stepped[0] += int(tr["n_stepped"].sum().item())
    env.set_lanes(1)
    for i in range(1):
        loop(i)
    stepped[0] = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.loop_batches):
        loop(i)
    torch.cuda.synchronize()
    rows["torch_loop"] = {"env_steps_per_s": stepped[0] / (time.perf_counter() - t0), "batches": args.loop_batches}
    mean_a = sum(a) / len(a)
    rows["rollout"] = {"env_steps_per_s": mean_a, "repeats": a, "spread": (max(a) - min(a)) / mean_a}
    b, d = rows["rl_record"]["env_steps_per_s"], rows["torch_loop"]["env_steps_per_s"]
    return {"policy": kind, "rows": rows, "ring_bytes": ring_bytes, "slots": G, "capacity_flagged_envs": flagged,
            "rl_record_vs_rollout": b / mean_a, "rl_record_noise_vs_rollout": rows["rl_record_noise"]["env_steps_per_s"] / mean_a, "rl_record_vs_torch_loop": b / d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="WPS_hard_x2")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-batches", type=int, default=3)
    ap.add_argument("--interval", type=int, default=20)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--weights", default="init2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    summary = {"case": args.case, "envs": args.envs, "interval": args.interval, "weights": args.weights, "steps": args.steps, "warmup": args.warmup, "policies": {}}
    for kind in ("pair", "context"):
        summary["policies"][kind] = measure(kind, args)
        print(json.dumps(summary["policies"][kind]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
