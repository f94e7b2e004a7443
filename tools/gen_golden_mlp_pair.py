#!/usr/bin/env python3
"""Golden vectors of the learned MLP-Pair hybrid, by RUNNING the reference (builder's container only; data only is written).

    python tools/gen_golden_mlp_pair.py [weights] [traces] [metrics]

PairCostHybrid(use_attention=False) (TaskAllocation/Hybrid/PairCostHybrid.py:154-197,266-278,308-328) on the CPU in torch float32,
driven by the evaluation harness's loop (experiments/wps_eval.py:244-254: _should_replan with interval 15) and by the trainer's
periodic evaluation (experiments/train_pair_cost.py:73-93, eval_local_swps: interval 20), over the reference env built as
tools/gen_golden.py builds it.  Output under tests/golden/:

  mlppair_weights_<set>.npz            w0 b0 w1 b1 w2 b2 (state_dict layout), raw_features, score_clamp
      init2      torch's default init under torch.manual_seed(7), every pair_mlp parameter x 2 (logits span about +-0.8 on the WPS cases)
      init2_raw  the same with raw_features=True (seed 8)
      il3        3 imitation episodes of train_pair_cost.run_il_episode on WPS_hard from the default init (seed 9)
  mlppair_trace_<tag>_s<seed>.npz      one episode, per plan: step, tf / af / tid / aid / ev (the tokens), torch's float32 scores and
                                       logits, scores64 (tests/policy_mlp_py.forward64: the same net on the same tokens in float64),
                                       selected (_selected_mask), pairs, actions; per step replanned; the 30 metrics, hung.n_replans
                                       (the HungarianAllocator's counter) and policy.n_replans (non-empty results only)
  mlppair_metrics_<tag>.npz            per seed: metrics32 / n_replans32 with the policy's own float32 scores, metrics64 / n_replans64
                                       with scores64 cast to float32 and passed through plan(scores=...)
<tag> = <case> for weight set init2 under the wps_eval loop, <case>__<set>_i<interval> otherwise; every file names its case,
weight set and interval.  The run ends with the condition the GPU test's cap rests on: over the init2 / interval-15 metrics files,
E >= 48 episodes over >= 3 cases and F_ref (episodes whose metrics32 != metrics64) <= E / 10.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

from gen_golden import METRIC_KEYS, OUT, _ids, make_env  # noqa: E402  (installs refshim)

import torch  # noqa: E402

import experiments.train_pair_cost as T  # noqa: E402
import experiments.wps_eval as W  # noqa: E402
import TaskAllocation.OptimizationBased.HungarianAllocator as HA  # noqa: E402
from experiments.paper_eval import _events  # noqa: E402
from TaskAllocation.Hybrid.PairCostHybrid import PairCostHybrid  # noqa: E402

import policy_mlp_py as twin  # noqa: E402

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
# tag suffix, weight set, interval, loop
MAIN = ("init2", 15)
TRACES = [("WPS_hard", "init2", 15, 0), ("WPS_hard_x2", "init2", 15, 0), ("WPS_attn", "init2", 15, 0), ("WPS_escort24", "init2", 15, 0),
          ("WPS_burst64", "init2", 15, 0), ("WPS_hard", "init2_raw", 20, 1), ("WPS_hard_x2", "il3", 20, 1), ("WPS_burst64", "init2_raw", 20, 1)]
METRICS = [("WPS_hard", "init2", 15, 16), ("WPS_hard_x2", "init2", 15, 16), ("WPS_attn", "init2", 15, 16),
           ("WPS_hard", "init2_raw", 20, 8), ("WPS_hard_x2", "il3", 20, 8)]


def tag_of(case, wset, interval):
    return case if (wset, interval) == MAIN else f"{case}__{wset}_i{interval}"


def seed_all(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def new_policy(raw):
    return PairCostHybrid(use_attention=False, max_tasks=32, max_agents=16, raw_features=raw, device="cpu")


def weights_of(policy):
    sd = policy.net.state_dict()
    w = {k: sd[f"pair_mlp.{i}.{p}"].detach().cpu().numpy().astype(np.float32).copy()
         for k, (i, p) in zip(KEYS, ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"), (4, "weight"), (4, "bias")))}
    w["raw_features"] = bool(policy.raw_features)
    w["score_clamp"] = float(policy.score_clamp)
    return w


def gen_weights():
    for name, raw, seed in (("init2", False, 7), ("init2_raw", True, 8)):
        seed_all(seed)
        p = new_policy(raw)
        with torch.no_grad():
            for q in p.net.pair_mlp.parameters():
                q.mul_(2.0)
        save_weights(name, weights_of(p))
    seed_all(9)
    p = new_policy(False)
    env = make_env("WPS_hard")
    hl = HA.HungarianAllocator(replan_interval=20, max_coord=env.max_coord)
    hg = HA.HungarianAllocator(replan_interval=20, max_coord=env.max_coord)
    for ep in range(3):
        loss = T.run_il_episode(env, p, hl, hg, il_batch=16)
        print("il episode", ep, "loss", loss, flush=True)
    p.imitation_flush()
    save_weights("il3", weights_of(p))


def save_weights(name, w):
    path = os.path.join(OUT, f"mlppair_weights_{name}.npz")
    np.savez_compressed(path, **{k: w[k] for k in KEYS}, raw_features=np.bool_(w["raw_features"]), score_clamp=np.float64(w["score_clamp"]))
    print(path, os.path.getsize(path), "B", flush=True)


def load_policy(name):
    w = twin.load_weights(twin.PAIR, name)
    p = new_policy(w["raw_features"])
    p.score_clamp = w["score_clamp"]
    sd = p.net.state_dict()
    for k, (i, q) in zip(KEYS, ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"), (4, "weight"), (4, "bias"))):
        sd[f"pair_mlp.{i}.{q}"] = torch.from_numpy(w[k].copy())
    p.net.load_state_dict(sd)
    return p, w


def run_episode(case, seed, policy, w, interval, use64, record):
    """interval 15: wps_eval.run_wps_episode's MLP-Pair branch (:244-248); interval 20: train_pair_cost.eval_local_swps (:73-93)."""
    env = make_env(case)
    hung = HA.HungarianAllocator(replan_interval=20, max_coord=env.max_coord)
    policy.n_replans = 0
    should, apply = (W._should_replan, W._apply_assign) if interval == 15 else (T._should_replan, T._apply_assign)
    obs, info = env.reset(seed=seed)
    done = {a: False for a in env.agents}
    trunc = {a: False for a in env.agents}
    rec = {k: [] for k in ("step", "tf", "af", "tid", "aid", "ev", "scores", "logits", "scores64", "selected")}
    pairs, acts, replanned, latest = [], [], [], None
    while not all(done.values()) and not all(trunc.values()):
        events = _events(info)
        actions = {}
        rp = bool(should(env, events, interval))
        replanned.append(int(rp))
        if rp:
            s_in = None
            if use64 or record:
                tok0 = policy.build_tokens(env)
                s64, _ = twin.forward64(twin.PAIR, w, tok0)
                if use64:
                    s_in = s64.astype(np.float32)
            result, tok, scores, noise, logits, selected = policy.plan(env, hung, events=events, explore=False, force=True, scores=s_in)
            actions = apply(env, result)
            if record:
                tid, aid = _ids(tok, 32, 16)
                for k, v in zip(rec, (env.time_steps, tok["task_feats"], tok["agent_feats"], tid, aid, tok["edge_valid"], scores, logits, s64, selected)):
                    rec[k].append(np.asarray(v).copy())
                for name, task in result:
                    pairs.append((env.time_steps, env.agent_by_name[name].id, task.id))
                for name, idx in actions.items():
                    acts.append((env.time_steps, env.agent_by_name[name].id, idx))
        obs, reward, done, trunc, info = env.step(actions)
        if isinstance(info, dict) and "metrics" in info:
            latest = info["metrics"]
    out = {"metrics": np.array([float(latest[k]) for k in METRIC_KEYS]), "n_replans": np.int64(hung.n_replans),
           "policy_n_replans": np.int64(policy.n_replans)}
    if record:
        out.update({k: np.stack(v) for k, v in rec.items()})
        out.update(pairs=np.array(pairs, dtype=np.int64).reshape(-1, 3), actions=np.array(acts, dtype=np.int64).reshape(-1, 3),
                   replanned=np.array(replanned, dtype=np.int64))
    return out


def gen_traces():
    for case, wset, interval, seed in TRACES:
        policy, w = load_policy(wset)
        tr = run_episode(case, seed, policy, w, interval, False, True)
        tr.update(case=np.array(case), weights=np.array(wset), interval=np.int64(interval), seed=np.int64(seed))
        path = os.path.join(OUT, f"mlppair_trace_{tag_of(case, wset, interval)}_s{seed}.npz")
        np.savez_compressed(path, **tr)
        ev = tr["ev"] != 0
        d_ref = float(np.abs(tr["scores"].astype(np.float64) - tr["scores64"])[ev].max()) if ev.any() else 0.0
        print(path, os.path.getsize(path), "B  plans", len(tr["step"]), "valid share", float(ev.mean()), "logit span", float(tr["logits"][ev].min()),
              float(tr["logits"][ev].max()), "D_ref", d_ref, "S_WPS", tr["metrics"][4], "replans", int(tr["n_replans"]), int(tr["policy_n_replans"]), flush=True)


def gen_metrics():
    E = F = 0
    cases = set()
    for case, wset, interval, n in METRICS:
        policy, w = load_policy(wset)
        cols = {k: [] for k in ("metrics32", "n_replans32", "policy_n_replans32", "metrics64", "n_replans64")}
        for s in range(n):
            a = run_episode(case, s, policy, w, interval, False, False)
            b = run_episode(case, s, policy, w, interval, True, False)
            cols["metrics32"].append(a["metrics"]); cols["n_replans32"].append(int(a["n_replans"])); cols["policy_n_replans32"].append(int(a["policy_n_replans"]))
            cols["metrics64"].append(b["metrics"]); cols["n_replans64"].append(int(b["n_replans"]))
        m32, m64 = np.stack(cols["metrics32"]), np.stack(cols["metrics64"])
        differ = np.array([not (np.array_equal(m32[i], m64[i]) and cols["n_replans32"][i] == cols["n_replans64"][i]) for i in range(n)])
        path = os.path.join(OUT, f"mlppair_metrics_{tag_of(case, wset, interval)}.npz")
        np.savez_compressed(path, metrics32=m32, metrics64=m64, n_replans32=np.array(cols["n_replans32"], dtype=np.int64),
                            n_replans64=np.array(cols["n_replans64"], dtype=np.int64), policy_n_replans32=np.array(cols["policy_n_replans32"], dtype=np.int64),
                            case=np.array(case), weights=np.array(wset), interval=np.int64(interval), keys=np.array(METRIC_KEYS))
        print(path, "mean S_WPS", m32[:, 4].mean(), "F_ref", int(differ.sum()), "of", n, flush=True)
        if (wset, interval) == MAIN:
            E += n; F += int(differ.sum()); cases.add(case)
    print(f"condition of the episode test: E = {E} over {len(cases)} cases, F_ref = {F}")
    assert E >= 48 and len(cases) >= 3 and F * 10 <= E, "the fixtures do not meet E >= 48 over >= 3 cases with F_ref <= E / 10"


def main():
    what = [a for a in sys.argv[1:]] or ["weights", "traces", "metrics"]
    if "weights" in what:
        gen_weights()
    if "traces" in what:
        gen_traces()
    if "metrics" in what:
        gen_metrics()


if __name__ == "__main__":
    main()
