#!/usr/bin/env python3
"""Golden vectors of the learned MLP-Coalition allocator, by RUNNING the reference (builder's container only; data only is written).

    python tools/gen_golden_mlp_coalition.py [weights] [traces] [metrics]

AttentionEscort(use_attention=False) (TaskAllocation/Hybrid/AttentionEscort.py:326-367,370-524) on the CPU in torch float32, driven by the
loop of experiments/escort_eval.run_escort_episode's MLP-Coalition branch (:181-188: _should_replan(env, events, interval), hung_force =
HungarianAllocator(replan_interval=10**9)) over the reference env built as tools/gen_golden.py builds it.  The sibling of
tools/gen_golden_mlp_context_pair.py.  Output under tests/golden/:

  mlpcoal_weights_<set>.npz            pair_mlp only: w0 [256, 38] b0 w1 b1 w2 b2 (state_dict layout)
      init2   torch's default init under torch.manual_seed(7), every pair_mlp parameter x 2
      ac3     3 episodes of experiments/train_escort.run_episode(explore=True) on WPS_escort from the default init (seed 9)
      wide    layer 3 only (w2, b2; the rest is init2's, `base`): init2's layer 3 x WIDE_SCALE with the bias moved so that the logits of
              init2's WPS_escort trace are centred — logits beyond +-20 on both sides and inside +-1 (asserted below)
  mlpcoal_trace_<tag>_s<seed>.npz      one episode, per plan: step, tf / af / tid / aid / tmask / amask / ev (the tokens), the policy's float32
                                       scores and logits (AttentionEscort.act, explore=False), scores64 (tests/policy_mlp_py.forward64 on
                                       the same float32 tokens), selected (_selected_mask), commit_until (every agent, after the plan), pairs,
                                       actions; per step replanned; the 30 metrics and hung_force.n_replans; d_ref = max |scores - scores64|
                                       over the valid pairs
  mlpcoal_metrics_<tag>.npz            per seed: metrics32 / n_replans32 with the policy's float32 scores, metrics64 / n_replans64 with
                                       scores64 cast to float32 and passed through _plan_from_scores
<tag> = <case> for weight set init2, <case>__<set> otherwise; interval 12 throughout.  The run ends with the condition the GPU test's cap
rests on: over the init2 metrics files, E >= 48 episodes over >= 3 cases and F_ref (episodes whose metrics32 != metrics64) <= E / 10.
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

import experiments.escort_eval as E  # noqa: E402
import experiments.train_escort as TE  # noqa: E402
import TaskAllocation.OptimizationBased.HungarianAllocator as HA  # noqa: E402
from experiments.paper_eval import _events  # noqa: E402
from TaskAllocation.Hybrid.AttentionEscort import AttentionEscort  # noqa: E402

import policy_mlp_py as twin  # noqa: E402

KEYS = twin.KEYS
SD = ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"), (4, "weight"), (4, "bias"))
INTERVAL = 12
WIDE_SCALE = 96.0
TRACES = [("WPS_escort", "init2", 0), ("WPS_escort24", "init2", 0), ("WPS_hard", "init2", 0), ("WPS_burst64", "init2", 0), ("WPS_escort", "ac3", 1)]
METRICS = [("WPS_escort", "init2", 16), ("WPS_escort24", "init2", 16), ("WPS_hard", "init2", 16), ("WPS_escort", "ac3", 8)]


def tag_of(case, wset):
    return case if wset == "init2" else f"{case}__{wset}"


def seed_all(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def new_policy():
    p = AttentionEscort(use_attention=False, max_tasks=twin.COALITION.max_tasks, max_agents=twin.COALITION.max_agents, device="cpu")
    p.eps = 0.0
    return p


def weights_of(policy):
    sd = policy.net.state_dict()
    return {k: sd[f"pair_mlp.{i}.{p}"].detach().cpu().numpy().astype(np.float32).copy() for k, (i, p) in zip(KEYS, SD)}


def save_weights(name, w):
    path = os.path.join(OUT, f"mlpcoal_weights_{name}.npz")
    np.savez_compressed(path, **w)
    print(path, os.path.getsize(path), "B", flush=True)


def gen_weights():
    seed_all(7)
    p = new_policy()
    with torch.no_grad():
        for q in p.net.pair_mlp.parameters():
            q.mul_(2.0)
    save_weights("init2", weights_of(p))
    seed_all(9)
    p = new_policy()
    p.eps = 0.2
    env = make_env("WPS_escort")
    for ep in range(3):
        hung = HA.HungarianAllocator(replan_interval=10**9, max_coord=env.max_coord)
        print("actor-critic episode", ep, TE.run_episode(env, p, hung, explore=True), "updates", p.n_updates, flush=True)
    save_weights("ac3", weights_of(p))


def load_weights(name):
    z = np.load(os.path.join(OUT, f"mlpcoal_weights_{name}.npz"))
    if "base" in z.files:
        w = load_weights(str(z["base"]))
        w["w2"], w["b2"] = np.ascontiguousarray(z["w2"], np.float32), np.ascontiguousarray(z["b2"], np.float32)
        return w
    return {k: np.ascontiguousarray(z[k], np.float32) for k in KEYS}


def load_policy(name):
    w = load_weights(name)
    p = new_policy()
    sd = p.net.state_dict()
    for k, (i, q) in zip(KEYS, SD):
        sd[f"pair_mlp.{i}.{q}"] = torch.from_numpy(w[k].copy())
    p.net.load_state_dict(sd)
    return p, w


def run_episode(case, seed, policy, w, use64, record):
    """run_escort_episode's MLP-Coalition branch; plan() taken apart (build_tokens, act, _plan_from_scores, _selected_mask) so that the
    float64 runs can hand their scores to _plan_from_scores — AttentionEscort.plan takes no scores="""
    env = make_env(case)
    obs, info = env.reset(seed=seed)
    hung_force = HA.HungarianAllocator(replan_interval=10**9, max_coord=env.max_coord)
    done = {a: False for a in env.agents}
    trunc = {a: False for a in env.agents}
    rec = {k: [] for k in ("step", "tf", "af", "tid", "aid", "tmask", "amask", "ev", "scores", "logits", "scores64", "selected", "commit_until")}
    pairs, acts, replanned, latest = [], [], [], None
    while not all(done.values()) and not all(trunc.values()):
        events = _events(info)
        actions = {}
        rp = bool(E._should_replan(env, events, INTERVAL))
        replanned.append(int(rp))
        if rp:
            tok = policy.build_tokens(env)
            scores, noise, logits = policy.act(tok, explore=False)
            s64 = None
            if use64 or record:
                s64, _ = twin.forward64(twin.COALITION, w, tok)
            result = policy._plan_from_scores(env, hung_force, tok, s64.astype(np.float32) if use64 else scores, events=events, force=True)
            actions = E._apply_assign(env, result)
            if record:
                tid, aid = _ids(tok, twin.COALITION.max_tasks, twin.COALITION.max_agents)
                commit = np.array([int(getattr(a, "commit_until", 0) or 0) for a in sorted(env.agents_obj, key=lambda u: u.id)], dtype=np.int64)
                ok = twin.cells(twin.COALITION, tok)
                for k, v in zip(rec, (env.time_steps, tok["task_feats"], tok["agent_feats"], tid, aid, np.asarray(tok["task_mask"], np.uint8),
                                         np.asarray(tok["agent_mask"], np.uint8), tok["edge_valid"], scores, logits * ok, s64, policy._selected_mask(tok, result), commit)):
                    rec[k].append(np.asarray(v).copy())
                for name, task in result:
                    pairs.append((env.time_steps, env.agent_by_name[name].id, task.id))
                for name, idx in actions.items():
                    acts.append((env.time_steps, env.agent_by_name[name].id, idx))
        obs, reward, done, trunc, info = env.step(actions)
        if isinstance(info, dict) and "metrics" in info:
            latest = info["metrics"]
    out = {"metrics": np.array([float(latest[k]) for k in METRIC_KEYS]), "n_replans": np.int64(hung_force.n_replans)}
    if record:
        out.update({k: np.stack(v) for k, v in rec.items()})
        out.update(pairs=np.array(pairs, dtype=np.int64).reshape(-1, 3), actions=np.array(acts, dtype=np.int64).reshape(-1, 3),
                   replanned=np.array(replanned, dtype=np.int64))
    return out


def valid_of(tr):
    return (tr["ev"] != 0) & (tr["amask"] == 0)[:, :, None] & (tr["tmask"] == 0)[:, None, :]


def gen_traces():
    for case, wset, seed in TRACES:
        policy, w = load_policy(wset)
        tr = run_episode(case, seed, policy, w, False, True)
        tr.update(case=np.array(case), weights=np.array(wset), interval=np.int64(INTERVAL), seed=np.int64(seed))
        path = os.path.join(OUT, f"mlpcoal_trace_{tag_of(case, wset)}_s{seed}.npz")
        ok = valid_of(tr)
        assert np.array_equal(ok, tr["ev"] != 0), "edge_valid is 0 on every pad pair"
        d_ref = float(np.abs(tr["scores"].astype(np.float64) - tr["scores64"])[ok].max()) if ok.any() else 0.0
        tr["d_ref"] = np.float64(d_ref)
        np.savez_compressed(path, **tr)
        print(path, os.path.getsize(path), "B  plans", len(tr["step"]), "valid share", float(ok.mean()), "max valid pairs", int(ok.sum(axis=(1, 2)).max()),
              "logit span", float(tr["logits"][ok].min()), float(tr["logits"][ok].max()), "D_ref", d_ref, "S_ESC", tr["metrics"][5], "replans", int(tr["n_replans"]), flush=True)


def gen_wide():
    """after the traces: centre init2's logits of the WPS_escort trace, scale layer 3"""
    tr = np.load(os.path.join(OUT, "mlpcoal_trace_WPS_escort_s0.npz"))
    ok = valid_of(tr)
    lg = tr["logits"][ok].astype(np.float64)
    mid = round(float((lg.min() + lg.max()) / 2), 2)
    w = load_weights("init2")
    w2 = (w["w2"] * np.float32(WIDE_SCALE)).astype(np.float32)
    b2 = ((w["b2"].astype(np.float64) - mid) * WIDE_SCALE).astype(np.float32)
    wide = dict(w, w2=w2, b2=b2)
    lo = hi = 0.0
    small = False
    for k in range(len(tr["step"])):
        _, l32 = twin.forward(twin.COALITION, wide, twin.trace_tokens(tr, k))
        v = l32[ok[k]]
        if len(v):
            lo, hi, small = min(lo, float(v.min())), max(hi, float(v.max())), small or bool((np.abs(v) < 1).any())
    print("wide: layer 3 x", WIDE_SCALE, "centre", mid, "logit span", lo, hi, "some |logit| < 1:", small, flush=True)
    assert lo < -20 and hi > 20 and small, "the wide set must reach both clip sides and the middle"
    path = os.path.join(OUT, "mlpcoal_weights_wide.npz")
    np.savez_compressed(path, w2=w2, b2=b2, base=np.array("init2"), scale=np.float64(WIDE_SCALE), centre=np.float64(mid))
    print(path, os.path.getsize(path), "B", flush=True)


def gen_metrics():
    Etot = F = 0
    cases = set()
    for case, wset, n in METRICS:
        policy, w = load_policy(wset)
        cols = {k: [] for k in ("metrics32", "n_replans32", "metrics64", "n_replans64")}
        for s in range(n):
            a = run_episode(case, s, policy, w, False, False)
            b = run_episode(case, s, policy, w, True, False)
            cols["metrics32"].append(a["metrics"]); cols["n_replans32"].append(int(a["n_replans"]))
            cols["metrics64"].append(b["metrics"]); cols["n_replans64"].append(int(b["n_replans"]))
        m32, m64 = np.stack(cols["metrics32"]), np.stack(cols["metrics64"])
        differ = np.array([not (np.array_equal(m32[i], m64[i]) and cols["n_replans32"][i] == cols["n_replans64"][i]) for i in range(n)])
        path = os.path.join(OUT, f"mlpcoal_metrics_{tag_of(case, wset)}.npz")
        np.savez_compressed(path, metrics32=m32, metrics64=m64, n_replans32=np.array(cols["n_replans32"], dtype=np.int64),
                            n_replans64=np.array(cols["n_replans64"], dtype=np.int64), case=np.array(case), weights=np.array(wset),
                            interval=np.int64(INTERVAL), keys=np.array(METRIC_KEYS))
        print(path, "mean S_ESC", m32[:, 5].mean(), "mean n_replans", np.mean(cols["n_replans32"]), "F_ref", int(differ.sum()), "of", n, flush=True)
        if wset == "init2":
            Etot += n; F += int(differ.sum()); cases.add(case)
    print(f"condition of the episode test: E = {Etot} over {len(cases)} cases, F_ref = {F}")
    assert Etot >= 48 and len(cases) >= 3 and F * 10 <= Etot, "the fixtures do not meet E >= 48 over >= 3 cases with F_ref <= E / 10"


def main():
    what = [a for a in sys.argv[1:]] or ["weights", "traces", "metrics"]
    if "weights" in what:
        gen_weights()
    if "traces" in what:
        gen_traces()
        gen_wide()
    if "metrics" in what:
        gen_metrics()


if __name__ == "__main__":
    main()
